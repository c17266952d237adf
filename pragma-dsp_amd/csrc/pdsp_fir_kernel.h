// pdsp_fir_kernel.h -- FIR filtering (linear convolution of real rows with one real filter) by overlap-save, fused
// into one launch: samples in, filtered samples out, nothing in between leaves LDS.
//
// One workgroup row owns one (signal row, block) pair of a plan of N = 2M points.  With P filter taps and
// hop = N - P + 1, block b of a row covers the input samples s ... s + N - 1, s = y_off + b*hop - (P - 1):
//   1. z[m] = x[s + 2m] + i x[s + 2m + 1] (zero outside [0, len)), Z = FFT_M(z)            -- the packed-real forward
//      of spectrum_packed_kernel / fft_real_kernel, on the same tables (Tables::tw_half, Tables::twr);
//   2. X[k] = (S - iP)/2, X[M-k] = conj(S + iP)/2 with S = Z[k] + conj Z[M-k], P = W_N^k (Z[k] - conj Z[M-k])
//      -- the Hermitian split, for the pair (k, M-k) one thread owns;
//   3. Y[k] = X[k] H[k], Y[M-k] = X[M-k] H[M-k]   (H: the filter's N-point spectrum, bins 0 ... M);
//   4. the inverse of the split: Z'[k] = A + i W_N^-k B, Z'[M-k] = conj(A) + i W_N^k conj(B) with A = Y[k] + conj Y[M-k],
//      B = Y[k] - conj Y[M-k], so that IFFT_M(Z'/2) = y[2m] + i y[2m+1] -- written back into the pair's own two LDS
//      slots (every slot has exactly one owner: no barrier between the reads and the writes);
//   5. IFFT_M as conj(FFT_M(conj(.))) / M: the pack stores conj(Z') / N (the 1/2 and the 1/M in one power of two),
//      the forward passes run again on the same registers twiddles and LDS, the result comes back in registers;
//   6. samples P-1 ... N-1 of the block (the circular wrap of the first P-1 is discarded) go to
//      y[b*hop + n - (P-1)], n < N, clamped to y_len.
// HBM traffic: N/hop reads + 1 write per output sample (the H bins and twiddles are L2-resident).
#pragma once

#include "pdsp_fft_kernel.h"

namespace pdsp {

// Rows of `len` real samples at stride x_stride; `items` = batch * nblk (row, block) pairs, item = row * nblk + b.
//   p1 = P - 1, hop = N - P + 1; y_off is the first output index (counted in the full convolution), y_len outputs
//   per row at stride y_stride.  h_re / h_im: N/2 + 1 bins.  g = 1 / (2N).
//   FAST: x and y 8-byte aligned with even strides, even hop and even y_off - p1: whole blocks inside [0, len) take
//         8-byte loads and pairs of outputs 8-byte stores; blocks at the ends of a row take the clamped path.
template <typename T, int LOG2M, bool FAST>
__global__ void __launch_bounds__(kPackedWG<LOG2M>)
fir_overlap_save_kernel(const T *__restrict__ xin, const long long len, const long long x_stride,
                        const T *__restrict__ h_re, const T *__restrict__ h_im, const int p1, const int hop,
                        const long long nblk, const long long y_off, const long long y_len, T *__restrict__ yout,
                        const long long y_stride, const typename vec2<T>::type *__restrict__ tw,
                        const typename vec2<T>::type *__restrict__ twr, const T g, const long long items) {
  constexpr int LOG2E = packed_log2e(LOG2M);
  using TR = FftTraits<LOG2M, LOG2E>;
  constexpr int E = TR::E, TP = TR::TP, M = TR::N;
  static_assert(LOG2M >= 5 && LOG2E == 4, "packed path: TP >= 2, sixteen points per thread (W_N^(TP q) = W_32^q)");
  typedef T V2 __attribute__((ext_vector_type(2)));

  __shared__ cx<T> lds[TR::LDS_ELEMS];

  const int tid = (int)(threadIdx.x % TP);
  const int rloc = (int)(threadIdx.x / TP);
  const long long item_raw = (long long)blockIdx.x * TR::ROWS + rloc;
  const bool live = item_raw < items;
  // dead rows of the last workgroup recompute the last live pair and skip the stores: every thread reaches every
  // barrier (items < 2^31 is checked on the host)
  const long long item = uniform_row<TP>(live ? item_raw : items - 1);
  const long long row = item / nblk, b = item - row * nblk;
  cx<T> *const lrow = lds + rloc * TR::LROW;

  const T *const xrow = xin + (size_t)row * (size_t)x_stride;
  const long long s = y_off + b * (long long)hop - p1;  // first sample of the block; may be negative

  constexpr bool kRegTw = TP >= 16;
  std::conditional_t<kRegTw, RegTwiddles<T, LOG2M, LOG2E>, TableTwiddles<T, LOG2M, LOG2E>> twf;
  cx<T> x[E];
  if (FAST && s >= 0 && s + 2 * M <= len) {
    const cx<T> *const x2 = reinterpret_cast<const cx<T> *>(xrow + s);  // s even: 8-byte aligned
    static_for<E>([&](auto q) { x[q] = ld_stream(x2 + TP * q + (unsigned)tid); });
  } else {
    // clamped loads + selects over the block's valid range [lo, hi) (32-bit, block-relative; the range is never
    // empty: the host launches only blocks that hold an output, and those start below len and end above 0)
    const int lo = s < 0 ? (int)-s : 0, hi = len - s < 2 * M ? (int)(len - s) : 2 * M;
    const T *const xb = xrow + (s + lo);
    static_for<E>([&](auto q) {
      const int n0 = 2 * (tid + TP * q) - lo, n1 = n0 + 1, w = hi - lo;
      const int c0 = n0 < 0 ? 0 : (n0 < w ? n0 : w - 1), c1 = n1 < 0 ? 0 : (n1 < w ? n1 : w - 1);
      const T v0 = ld_stream(xb + c0), v1 = ld_stream(xb + c1);
      x[q] = cx<T>{(n0 >= 0 && n0 < w) ? v0 : T(0), (n1 >= 0 && n1 < w) ? v1 : T(0)};
    });
  }
  // the tables behind the row loads, as fft_real_kernel (load_order_fence's header)
  if constexpr (kRegTw) twf.load(reinterpret_cast<const cx<T> *>(tw), tid);
  else twf.tw = reinterpret_cast<const cx<T> *>(tw);
  const cx<T> twk0 = reinterpret_cast<const cx<T> *>(twr)[(unsigned)tid];  // W_N^tid; W_N^(tid + TP q) = twk0 W_32^q

  fft_passes<T, LOG2M, true, LOG2E>(x, lrow, twf, tid);  // Z in LDS, natural order
  __syncthreads();

  // pairs k = tid + TP q, q < E/2 (k < M/2); k = M/2 is one more pair for tid == 0 (it pairs with itself)
  static_for<E / 2 + 1>([&](auto qc) {
    constexpr int q = qc;
    if (q < E / 2 || tid == 0) {
      const int k = tid + TP * q, k2 = (M - k) & (M - 1);  // k = 0: Z[M] == Z[0]
      const cx<T> z = lrow[lds_pad(k)], zp = lrow[lds_pad(k2)];
      const cx<T> w = mul_w32<T, q>(twk0);  // W_N^k
      const cx<T> hk{h_re[k], h_im[k]}, hm{h_re[M - k], h_im[M - k]};
      const cx<T> sm = z + conj(zp), pm = cmul(z - conj(zp), w);
      const cx<T> ya = cmul(add_mul_neg_i(sm, pm), hk) * g;         // 2 X[k] H[k] / (2N)
      const cx<T> yb = cmul(conj(add_mul_pos_i(sm, pm)), hm) * g;   // 2 X[M-k] H[M-k] / (2N)  (k = 0: Nyquist)
      const cx<T> a = ya + conj(yb), c = cmul(ya - conj(yb), conj(w));  // A, W_N^-k B
      lrow[lds_pad(k)] = conj(add_mul_pos_i(a, c));                     // conj Z'[k] / N
      if (k != 0 && k2 != k) lrow[lds_pad(k2)] = add_mul_neg_i(a, c);   // conj Z'[M-k] / N
    }
  });
  __syncthreads();
  fft_pass_readback<T, LOG2M, LOG2E>(x, lrow, tid);
  __syncthreads();  // the first pass writes LDS again
  // conj(y[2m] + i y[2m+1]) in slot q, m = tid + TP q.  f64 reads the table at every use in this second transform
  // instead of keeping the register bases alive across the pack: 2 workgroups per CU instead of 1 (and no spills
  // at N = 16384)
  if constexpr (sizeof(T) == 8) {
    TableTwiddles<T, LOG2M, LOG2E> twt{reinterpret_cast<const cx<T> *>(tw)};
    fft_passes<T, LOG2M, false, LOG2E>(x, lrow, twt, tid);
  } else {
    fft_passes<T, LOG2M, false, LOG2E>(x, lrow, twf, tid);
  }

  if (!live) return;
  // 32-bit, block-relative output indices: sample n of the block is output b*hop + (n - p1), kept when p1 <= n and
  // n - p1 < rem
  T *const yb = yout + (size_t)row * (size_t)y_stride + b * (long long)hop;
  const long long rem_ll = y_len - b * (long long)hop;
  const int rem = rem_ll < 2 * M ? (int)rem_ll : 2 * M;
  static_for<E>([&](auto q) {
    const int n = 2 * (tid + TP * q), o = n - p1;
    const T v0 = x[q].x, v1 = -x[q].y;
    if (FAST && o >= 0 && o + 1 < rem) {
      __builtin_nontemporal_store(V2{v0, v1}, reinterpret_cast<V2 *>(yb + o));  // o even
    } else {
      if (o >= 0 && o < rem) yb[o] = v0;
      if (o + 1 >= 0 && o + 1 < rem) yb[o + 1] = v1;
    }
  });
}

// H[k] = sum_j taps[j] W_N^(j k), k = 0 ... N/2: one workgroup per bin, the taps split over its threads and summed in
// f64 with exact twiddle arguments ((j k) mod N is an integer), rounded once to T.  Runs once per filter.
template <typename T>
__global__ void __launch_bounds__(256)
fir_spectrum_kernel(const T *__restrict__ taps, const int ntaps, const int log2n, T *__restrict__ h_re,
                    T *__restrict__ h_im) {
  __shared__ double red[2][256];
  const long long k = blockIdx.x;
  const long long mask = (1LL << log2n) - 1;
  const double f = -2.0 / (double)(1LL << log2n);
  double re = 0.0, im = 0.0;
  for (int j = (int)threadIdx.x; j < ntaps; j += 256) {
    double sn, cs;
    sincospi(f * (double)(((long long)j * k) & mask), &sn, &cs);
    const double t = (double)taps[j];
    re = fma(t, cs, re);
    im = fma(t, sn, im);
  }
  red[0][threadIdx.x] = re;
  red[1][threadIdx.x] = im;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      red[0][threadIdx.x] += red[0][threadIdx.x + w];
      red[1][threadIdx.x] += red[1][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    h_re[k] = (T)red[0][0];
    h_im[k] = (T)red[1][0];
  }
}

}  // namespace pdsp

// pdsp_fir_kernel.h -- FIR filtering (linear convolution of real rows with one real filter) by overlap-save, fused
// into one launch: samples in, filtered samples out, nothing in between leaves LDS.
//
// One workgroup row owns one (signal row, block) pair of a plan of N = 2M points.  With P filter taps and
// hop = N - P + 1, block b of a row covers the input samples s ... s + N - 1, s = y_off + b*hop - (P - 1):
//   1. z[m] = x[s + 2m] + i x[s + 2m + 1] (zero outside [0, len)), Z = FFT_M(z), on the packed-real tables
//      (Tables::tw_half, Tables::twr);
//   2. 2 X[k], 2 X[M-k] by the forward split (pdsp_packed.h), times H[k] resp. H[M-k] / (2N) (H: the filter's
//      N-point spectrum, bins 0 ... M): Y / N;
//   3. the inverse split of Y / N into the row's LDS, and the second transform: y[2m] + i y[2m+1], conjugated, in
//      registers;
//   4. samples P-1 ... N-1 of the block (the circular wrap of the first P-1 is discarded) go to
//      y[b*hop + n - (P-1)], n < N, clamped to y_len.
// HBM traffic: N/hop reads + 1 write per output sample (the H bins and twiddles are L2-resident).
#pragma once

#include "pdsp_packed.h"

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
  using PR = PackedRow<T, LOG2M>;
  constexpr int E = PR::E, TP = PR::TP, M = PR::M;
  typedef T V2 __attribute__((ext_vector_type(2)));

  __shared__ cx<T> lds[PR::TR::LDS_ELEMS];
  const PR pr(lds, items);
  const int tid = pr.tid;
  const long long row = pr.row / nblk, b = pr.row - row * nblk;

  const T *const xrow = xin + (size_t)row * (size_t)x_stride;
  const long long s = y_off + b * (long long)hop - p1;  // first sample of the block; may be negative

  PackedTwiddles<T, LOG2M> twd;
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
  twd.load(tw, twr, tid);  // the tables behind the row loads, as fft_real_kernel (load_order_fence's header)

  fft_passes<T, LOG2M, true, PR::LOG2E>(x, pr.lrow, twd.twf, tid);  // Z in LDS, natural order
  __syncthreads();
  pr.for_each_pair([&](auto q, const int k) {
    const int k2 = (M - k) & (M - 1);
    const auto sp = pr.forward_split(k, k2);
    const cx<T> w = twd.wk(q);  // W_N^k
    const cx<T> hk{h_re[k], h_im[k]}, hm{h_re[M - k], h_im[M - k]};
    pr.inverse_split(k, k2, cmul(sp.x(w), hk) * g, cmul(sp.xm(w), hm) * g, w);  // Y / N; k = 0: xm is X[M]
  });
  // f64 reads the table at every use in the second transform instead of keeping the register bases alive across
  // the split: 2 workgroups per CU instead of 1 (and no spills at N = 16384)
  if constexpr (sizeof(T) == 8)
    pr.second_transform(x, TableTwiddles<T, LOG2M, PR::LOG2E>{reinterpret_cast<const cx<T> *>(tw)});
  else
    pr.second_transform(x, twd.twf);

  if (!pr.live) return;
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

// pdsp_stft_kernel.h -- the complex short-time transform and its overlap-add inverse, N = 2M = 64 ... 16384.
//
// Forward (stft_complex_kernel): one row = one frame b of `frame_len` samples at row stride h (overlapping frames of
// one signal are read in place, never materialised), zero-padded to N:
//   1. z[m] = w[2m] x[2m] + i w[2m+1] x[2m+1], Z = FFT_M(z)     -- the packed-real row of pdsp_packed.h;
//   2. X[k] and X[M-k], half the forward split of the pair (k, M-k), k = 0 ... M, to the planes re / im
//      [frame][M + 1] (unscaled: the one-sided DFT of w * frame).
// HBM traffic: N/h reads (h < N: L2 serves part of the overlap) + (N + 2)/N writes per input sample.
//
// Inverse, one frame (istft_frame_kernel): y_b = irfft(X_b, N), the imaginary parts of X[0] and X[M] ignored:
//   3. the inverse split of Y / N, the bins read from HBM, and the second transform (pdsp_packed.h): conj(y[2m] +
//      i y[2m+1]) in registers;
//   4. v[n] = w[n] y[n] in registers; then
//      DIRECT (h >= N: frames do not overlap): out[b h + n] = v / w[n]^2 if w[n]^2 > 1e-11, else 0, and the h - N gap
//             samples behind the frame (all but the last frame) are written as 0 -- one launch, no scratch;
//      else:  v[n] goes to scratch row (b - first) of N values.
// Overlap-add (istft_ola_kernel, h < N): one thread per output sample t gathers the frames that cover it,
//   b = ceil((t - N + 1) / h) ... min(F - 1, t / h), in ASCENDING b: num = sum v_b[t - b h], den = sum w[t - b h]^2,
//   out[t] = num / den if den > 1e-11, else 0.  No atomics: every output has one writer and a fixed order, so results
//   are bit-identical from call to call and for every chunk size.
// Chunking (host, pdsp_kernels_stft.hip): chunk c finalises outputs [c S h, (c + 1) S h) (the last one up to T) from
//   frames c S - K ... (c + 1) S - 1, K = ceil(N / h) - 1 frames recomputed before its start; scratch holds
//   min(S + K, F) N values, S >= K + 1: at most max(256 MiB, (2K + 1) N sizeof T) whatever F is.
#pragma once

#include "pdsp_packed.h"

namespace pdsp {

// den threshold of the overlap-add normalisation (torch.istft's NOLA bound)
constexpr double kIstftDenMin = 1e-11;

// frames: `batch` rows at `stride`; the first min(frame_len, N) samples of a row are used, zero beyond.
// win: N values or null (rect).  re / im: [batch][M + 1].
template <typename T, int LOG2M, bool HAS_WIN>
__global__ void __launch_bounds__(kPackedWG<LOG2M>)
stft_complex_kernel(const T *__restrict__ frames, const T *__restrict__ win, const long long frame_len,
                    const long long stride, const typename vec2<T>::type *__restrict__ tw,
                    const typename vec2<T>::type *__restrict__ twr, T *__restrict__ re_out, T *__restrict__ im_out,
                    const long long batch) {
  using PR = PackedRow<T, LOG2M>;
  constexpr int E = PR::E, TP = PR::TP, M = PR::M;

  __shared__ cx<T> lds[PR::TR::LDS_ELEMS];
  const PR pr(lds, batch);
  const int tid = pr.tid;
  const T *const xrow = frames + (size_t)pr.row * (size_t)stride;

  // tables first (load_order_fence's header): twiddle bases, the split twiddle, the thread's window values
  PackedTwiddles<T, LOG2M> twd;
  twd.load(tw, twr, tid);
  cx<T> wv[HAS_WIN ? E : 1];
  if constexpr (HAS_WIN)  // a window at any alignment: two scalar loads per pair
    static_for<E>([&](auto q) { wv[q] = cx<T>{(win + 2 * TP * q)[2 * (unsigned)tid], (win + 2 * TP * q + 1)[2 * (unsigned)tid]}; });
  load_order_fence();
  // clamped loads + selects over [0, flen), 1 <= flen <= N
  cx<T> x[E];
  const int flen = (int)frame_len;
  static_for<E>([&](auto q) {
    const int i0 = 2 * (tid + TP * q);
    const int c0 = i0 < flen - 1 ? i0 : flen - 1, c1 = i0 + 1 < flen - 1 ? i0 + 1 : flen - 1;
    const T v0 = ld_stream(xrow + (unsigned)c0), v1 = ld_stream(xrow + (unsigned)c1);
    x[q] = cx<T>{i0 < flen ? v0 : T(0), i0 + 1 < flen ? v1 : T(0)};
  });
  if constexpr (HAS_WIN) static_for<E>([&](auto q) { x[q] = x[q] * wv[q]; });

  fft_passes<T, LOG2M, true, PR::LOG2E>(x, pr.lrow, twd.twf, tid);  // Z in LDS, natural order
  __syncthreads();
  if (!pr.live) return;  // no barrier below

  T *const rrow = re_out + (size_t)pr.row * (size_t)(M + 1);
  T *const irow = im_out + (size_t)pr.row * (size_t)(M + 1);
  pr.for_each_pair([&](auto q, const int k) {
    const auto sp = pr.forward_split(k, (M - k) & (M - 1));
    const cx<T> w = twd.wk(q);  // W_N^k
    const cx<T> xa = sp.x(w) * T(0.5);   // X[k]
    const cx<T> xb = sp.xm(w) * T(0.5);  // X[M-k]  (k = 0: the Nyquist bin X[M])
    rrow[k] = xa.x;
    irow[k] = xa.y;
    if (k != M / 2) {
      rrow[M - k] = xb.x;
      irow[M - k] = xb.y;
    }
  });
}

// re / im: frames first ... first + items - 1 of M + 1 bins each (pointers at frame `first`).  g = 1 / N.
//   DIRECT: out is the whole output of T = (nframes - 1) h + N samples (h >= N); else out = scratch [items][N].
template <typename T, int LOG2M, bool HAS_WIN, bool DIRECT>
__global__ void __launch_bounds__(kPackedWG<LOG2M>)
istft_frame_kernel(const T *__restrict__ re_in, const T *__restrict__ im_in, const T *__restrict__ win,
                   const long long first, const long long items, const long long nframes, const long long hop,
                   T *__restrict__ out, const typename vec2<T>::type *__restrict__ tw,
                   const typename vec2<T>::type *__restrict__ twr, const T g) {
  using PR = PackedRow<T, LOG2M>;
  constexpr int E = PR::E, TP = PR::TP, M = PR::M;
  typedef T V2 __attribute__((ext_vector_type(2)));

  __shared__ cx<T> lds[PR::TR::LDS_ELEMS];
  const PR pr(lds, items);
  const int tid = pr.tid;
  const long long item = pr.row;
  const T *const rrow = re_in + (size_t)item * (size_t)(M + 1);
  const T *const irow = im_in + (size_t)item * (size_t)(M + 1);

  PackedTwiddles<T, LOG2M> twd;
  twd.load_split(twr, tid);
  // the inverse split straight from the bins
  pr.for_each_pair([&](auto q, const int k) {
    const int k2 = M - k;  // k = 0 pairs with the Nyquist bin M
    cx<T> ya{rrow[k], irow[k]}, yb{rrow[k2], irow[k2]};
    if (k == 0) ya.y = yb.y = T(0);  // irfft ignores the imaginary parts of bins 0 and M
    ya = ya * g;
    yb = yb * g;
    pr.inverse_split(k, k2, ya, yb, twd.wk(q));
  });
  twd.load_passes(tw, tid);
  cx<T> x[E];
  pr.second_transform(x, twd.twf);  // conj(y[2m] + i y[2m+1]) in slot q, m = tid + TP q

  if (!pr.live) return;
  const long long b = first + item;
  static_for<E>([&](auto q) {
    const int n = 2 * (tid + TP * q);
    T v0 = x[q].x, v1 = -x[q].y, d0 = T(1), d1 = T(1);
    if constexpr (HAS_WIN) {
      const T w0 = win[n], w1 = win[n + 1];
      v0 *= w0;
      v1 *= w1;
      d0 = w0 * w0;
      d1 = w1 * w1;
    }
    if constexpr (DIRECT) {
      T *const ob = out + b * hop + n;
      ob[0] = d0 > T(kIstftDenMin) ? v0 / d0 : T(0);
      ob[1] = d1 > T(kIstftDenMin) ? v1 / d1 : T(0);
    } else {
      *reinterpret_cast<V2 *>(out + (size_t)item * (size_t)(2 * M) + n) = V2{v0, v1};  // n even, N even: 8-byte aligned
    }
  });
  if constexpr (DIRECT) {
    if (b + 1 < nframes) {  // the gap [b h + N, (b + 1) h) is covered by no frame
      T *const gap = out + b * hop + 2 * M;
      for (long long j = tid; j < hop - 2 * M; j += TP) gap[j] = T(0);
    }
  }
}

// Outputs t0 ... t0 + count - 1 of the overlap-add (h < N); v: scratch rows of the frames first, first + 1, ...
template <typename T, bool HAS_WIN>
__global__ void __launch_bounds__(256)
istft_ola_kernel(const T *__restrict__ v, const T *__restrict__ win, const int n, const long long hop,
                 const long long nframes, const long long first, const long long t0, const long long count,
                 T *__restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const long long t = t0 + i;
  const long long lo_num = t - n + 1;
  const long long b_lo = lo_num > 0 ? (lo_num + hop - 1) / hop : 0;
  const long long b_top = t / hop, b_hi = b_top < nframes - 1 ? b_top : nframes - 1;
  T num = T(0), den = T(0);
  for (long long b = b_lo; b <= b_hi; ++b) {
    const int k = (int)(t - b * hop);
    num += v[(size_t)(b - first) * (size_t)n + (unsigned)k];
    if constexpr (HAS_WIN) {
      const T w = win[k];
      den += w * w;
    } else {
      den += T(1);
    }
  }
  out[t] = den > T(kIstftDenMin) ? num / den : T(0);
}

}  // namespace pdsp

// pdsp_czt_kernel.h -- the chirp-z transform of rows (scipy.signal.czt / zoom_fft along a row): K points of the
// z-transform of a row of L samples on an arc of a circle,
//   X[k] = sum_{n < L} x[n] a^-n w^(n k),  k < K,  w = exp(-2 pi i step),  a = radius exp(2 pi i start),
// fused into one launch.  It is bluestein_kernel's data flow (pdsp_bluestein_kernel.h: chirp product, forward pass set
// into LDS, pointwise product, second transform, chirp product) with the arc, the number of bins and the start point
// free: n k = (n^2 + k^2 - (k - n)^2) / 2 gives
//   X[k] = post[k] sum_n (x[n] pre[n]) b[k - n],  pre[n] = a^-n w^(n^2/2),  post[k] = w^(k^2/2),  b[j] = w^(-j^2/2),
// a convolution with the lags -(L - 1) ... K - 1, which a circular one of M >= L + K - 1 points holds.  One workgroup
// row owns one signal row:
//   1. u[m] = x[m] pre[m] for m < L, 0 up to M; U = FFT_M(u) into the row's LDS, natural order;
//   2. every thread multiplies its own E slots by Bt = FFT_M(b) / M (b[j] at j for j >= 0, at M + j for j < 0, zero
//      elsewhere) and writes the conjugate back (one owner per slot: no barrier between the read and the write);
//   3. the second transform (PackedRow::second_transform) leaves conj y[m] in the registers that held u[m];
//   4. X[m] = y[m] post[m], m < K.
// There is no inverse, so no sign and no scale.  pre (L entries), post (K entries) and Bt (M entries) are built in long
// double on the host with exactly reduced phases and rounded once; every row reads them and they stay in L2.
// HBM traffic: one read of the row and one write of its bins.  The exact in-place call is safe: a workgroup loads all
// of its rows in full before its first barrier and stores only into those rows.
#pragma once

#include "pdsp_packed.h"

namespace pdsp {

// re_in / im_in (im_in null: real rows): `batch` rows of `len` samples at in_stride; re_out / im_out: rows of `bins`
// points at out_stride.  len, bins >= 1, len + bins - 1 <= M.  tw: the radix table of the M-point transform (the
// tw_half of a plan of 2M points).
template <typename T, int LOG2M>
__global__ void __launch_bounds__(kPackedWG<LOG2M>)
czt_kernel(const T *re_in, const T *im_in, const long long in_stride, const int len, T *re_out, T *im_out,
           const long long out_stride, const int bins, const cx<T> *__restrict__ pre, const cx<T> *__restrict__ post,
           const cx<T> *__restrict__ bt, const typename vec2<T>::type *__restrict__ tw, const long long batch) {
  using PR = PackedRow<T, LOG2M>;
  constexpr int E = PR::E, TP = PR::TP;

  __shared__ cx<T> lds[PR::TR::LDS_ELEMS];
  const PR pr(lds, batch);
  const int tid = pr.tid;

  // slot q holds sample m = tid + TP q: clamped loads + selects over the valid range [0, len), len >= 1
  PackedTwiddles<T, LOG2M> twd;
  cx<T> x[E];
  {
    const T *const rrow = re_in + (size_t)pr.row * (size_t)in_stride;
    const T *const irow = im_in ? im_in + (size_t)pr.row * (size_t)in_stride : rrow;  // not read when im_in is null
    static_for<E>([&](auto q) {
      const int m = tid + TP * q;
      const unsigned cm = (unsigned)(m < len ? m : len - 1);
      const T vr = ld_stream(rrow + cm);
      const T vi = im_in ? ld_stream(irow + cm) : T(0);
      x[q] = cx<T>{m < len ? vr : T(0), m < len ? vi : T(0)};
    });
    twd.load_passes(tw, tid);  // the tables behind the row loads, as bluestein_kernel
    // real rows promise the bits of complex rows with a zero plane: the loaded values become opaque here, so the
    // arithmetic below compiles the same whichever way they came
    pin_regs<T, E>(x);
    static_for<E>([&](auto q) {
      const int m = tid + TP * q;
      x[q] = cmul(x[q], pre[(unsigned)(m < len ? m : len - 1)]);  // a zero slot stays zero: pre is finite
    });
  }

  fft_passes<T, LOG2M, true, PR::LOG2E>(x, pr.lrow, twd.twf, tid);  // U in LDS, natural order
  __syncthreads();
  {
    // this thread's own slots k = tid + TP q: conj(U[k] Bt[k])
    cx<T> *const own = pr.lrow + lds_pad(tid);
    static_for<E>([&](auto q) {
      const int k = tid + TP * q;
      cx<T> *const p = (TP % 16 == 0) ? own + cpad(TP * q) : pr.lrow + lds_pad(k);
      *p = conj(cmul(*p, bt[(unsigned)k]));
    });
  }
  // f64 reads the table at every use in the second transform, as bluestein_kernel does
  if constexpr (sizeof(T) == 8)
    pr.second_transform(x, TableTwiddles<T, LOG2M, PR::LOG2E>{reinterpret_cast<const cx<T> *>(tw)});
  else
    pr.second_transform(x, twd.twf);
  pin_regs<T, E>(x);

  if (!pr.live) return;
  // The epilogue's table and count pass through an empty asm, as bluestein_kernel's second chirp load does: the
  // compiler schedules these loads here, behind both transforms, instead of holding E values across them.
  const cx<T> *post2 = post;
  int bins2 = bins;
  asm volatile("" : "+s"(post2), "+s"(bins2));
  T *const rout = re_out + (size_t)pr.row * (size_t)out_stride;
  T *const iout = im_out + (size_t)pr.row * (size_t)out_stride;
  static_for<E>([&](auto q) {
    const int m = tid + TP * q;
    if (m < bins2) {
      const cx<T> v = cmul(conj(x[q]), post2[(unsigned)m]);
      rout[(unsigned)m] = v.x;
      iout[(unsigned)m] = v.y;
    }
  });
}

}  // namespace pdsp

// pdsp_bluestein_kernel.h -- the DFT of rows of ANY length L, 2 <= L <= 4096 (numpy.fft.fft / ifft along a row), by
// Bluestein's chirp-z algorithm, fused into one launch: samples in, bins out, nothing in between leaves LDS.  It is
// the Hilbert kernel's data flow (pdsp_hilbert_kernel.h: forward, pointwise, second transform) without the packed-real
// splits: the rows are complex, so the M-point transform is the row's own.
//
// With c[n] = exp(-i pi n^2 / L), n k = (n^2 + k^2 - (k - n)^2) / 2 turns the DFT into a convolution,
//   X[k] = c[k] sum_n (x[n] c[n]) conj c[k - n],
// which a circular convolution of M >= 2L - 1 points computes without aliasing.  One workgroup row owns one signal row:
//   1. a[m] = x[m] c[m] for m < L, 0 up to M; A = FFT_M(a) into the row's LDS, natural order;
//   2. every thread multiplies its own E slots by Bt = FFT_M(b) / M, b[j] = conj c[|j|] at j and M - j for |j| < L, and
//      writes the conjugate back (one owner per slot: no barrier between the read and the write);
//   3. the second transform (PackedRow::second_transform: IFFT_M = conj FFT_M conj / M) leaves conj y[m] in the
//      registers that held a[m];
//   4. X[m] = y[m] c[m], m < L.
// The inverse is the same launch with the input and the output conjugated and 1/L on the store: sgn = -1 multiplies
// both imaginary parts (exact), g = 1/L (forward: 1, exact) every output.  c (L entries) and Bt (M entries) are built
// in f64 on the host and rounded once; every row reads them and they stay in L2.
// HBM traffic: one read and one write of the row.  The exact in-place call is safe: a row is loaded in full by its own
// workgroup before that workgroup's first barrier, and each thread stores only the m it loaded.
#pragma once

#include "pdsp_packed.h"

namespace pdsp {

// re_in / im_in (im_in null: real rows): `batch` rows of `len` points at in_stride; re_out / im_out at out_stride.
// tw: the radix table of the M-point transform (the tw_half of a plan of 2M points).
template <typename T, int LOG2M>
__global__ void __launch_bounds__(kPackedWG<LOG2M>)
bluestein_kernel(const T *re_in, const T *im_in, const long long in_stride, const int len, T *re_out, T *im_out,
                 const long long out_stride, const cx<T> *__restrict__ chirp, const cx<T> *__restrict__ bt,
                 const typename vec2<T>::type *__restrict__ tw, const T sgn, const T g, const long long batch) {
  using PR = PackedRow<T, LOG2M>;
  constexpr int E = PR::E, TP = PR::TP;

  __shared__ cx<T> lds[PR::TR::LDS_ELEMS];
  const PR pr(lds, batch);
  const int tid = pr.tid;

  // slot q holds point m = tid + TP q: clamped loads + selects over the valid range [0, len), len >= 2
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
    twd.load_passes(tw, tid);  // the tables behind the row loads, as hilbert_kernel
    // real rows promise the bits of complex rows with a zero plane: the loaded values become opaque here, so the
    // arithmetic below compiles the same whichever way they came
    pin_regs<T, E>(x);
    static_for<E>([&](auto q) {
      const int m = tid + TP * q;
      const cx<T> c = chirp[(unsigned)(m < len ? m : len - 1)];
      x[q] = cmul(cx<T>{x[q].x, x[q].y * sgn}, c);  // a zero slot stays zero
    });
  }

  fft_passes<T, LOG2M, true, PR::LOG2E>(x, pr.lrow, twd.twf, tid);  // A in LDS, natural order
  __syncthreads();
  {
    // this thread's own slots k = tid + TP q: conj(A[k] Bt[k])
    cx<T> *const own = pr.lrow + lds_pad(tid);
    static_for<E>([&](auto q) {
      const int k = tid + TP * q;
      cx<T> *const p = (TP % 16 == 0) ? own + cpad(TP * q) : pr.lrow + lds_pad(k);
      *p = conj(cmul(*p, bt[(unsigned)k]));
    });
  }
  // f64 reads the table at every use in the second transform, as hilbert_kernel does
  if constexpr (sizeof(T) == 8)
    pr.second_transform(x, TableTwiddles<T, LOG2M, PR::LOG2E>{reinterpret_cast<const cx<T> *>(tw)});
  else
    pr.second_transform(x, twd.twf);
  pin_regs<T, E>(x);

  if (!pr.live) return;
  // The chirp is loaded AGAIN: left alone the compiler keeps the E values of step 1 in registers across both
  // transforms.  The table's address and len pass through an empty asm, so the second loads are not the first ones to
  // the compiler (hilbert_kernel's second row load).
  const cx<T> *chirp2 = chirp;
  int len2 = len;
  asm volatile("" : "+s"(chirp2), "+s"(len2));
  T *const rout = re_out + (size_t)pr.row * (size_t)out_stride;
  T *const iout = im_out + (size_t)pr.row * (size_t)out_stride;
  const T gi = g * sgn;
  static_for<E>([&](auto q) {
    const int m = tid + TP * q;
    if (m < len2) {
      const cx<T> v = cmul(conj(x[q]), chirp2[(unsigned)m]);
      rout[(unsigned)m] = v.x * g;
      iout[(unsigned)m] = v.y * gi;
    }
  });
}

}  // namespace pdsp

// pdsp_dct_kernel.h -- DCT-II and DCT-III of rows of N = 2M = 64 ... 16384 real values (scipy dct / idct,
// types 2 and 3), one row per TP = M/16 threads, one launch per call, N values in and N values out per row.
//
// DCT-II (dct2_kernel), Makhoul's algorithm on the packed-real row of pdsp_packed.h:
//   1. v[n] = x[2n], v[N-1-n] = x[2n+1] (n < M), packed z[m] = v[2m] + i v[2m+1]: for m < M/2
//      z[m] = x[4m] + i x[4m+2] and z[M-1-m] = x[4m+3] + i x[4m+1] -- one quad x[4m ... 4m+3] feeds slot q of thread
//      tid (m = tid + TP q) and slot E-1-q of thread TP-1-tid;
//   2. V = rfft(v), bins k and M-k from the forward split of Z = FFT_M(z);
//   3. c_k = W_4N^k V[k]: y[k] = 2 Re c_k, y[N-k] = -2 Im c_k.  The thread that owns the pair (k, M-k) writes y[k],
//      y[N-k], y[M-k], y[M+k]; k = 0 gives y[0] and y[M], k = M/2 (its own partner) y[M/2] and y[3M/2].
// DCT-III (dct3_kernel), the mirror:
//   4. V[k] = conj(W_4N^k) (y[k] - i y[N-k]), y[N] := 0, k = 0 ... M (V[0], V[M] real: their imaginary parts are
//      dropped), the inverse split of the pair (k, M-k) into the row's LDS;
//   5. the second transform gives conj(v[2m] + i v[2m+1]), v = N irfft(V) = 2N idct-II(y);
//   6. x[2n] = v[n], x[2n+1] = v[N-1-n]: slot q of m < M/2 goes to x[4m], x[4m+2], of m >= M/2 to x[4m'+3], x[4m'+1],
//      m' = M-1-m.
// Norms: every output of the DCT-II is scaled by g and y[0] by g0 instead; every input of the DCT-III by g and y[0]
// by g0 instead (the host folds scipy's norm into the two, pdsp_kernels_dct.hip).
// FAST (row pointers 16-byte aligned, strides multiples of 16 bytes): the rows move as 16-byte quads, exchanged
// through the row's LDS as N plain values (step 1's quads into slot order; step 3's outputs and step 6's inputs of
// the DCT-III into quads).  The general path reads and writes single values where steps 1, 3, 4 and 6 put them.
// Exact in place (y == x, same stride) is safe on both: a row is loaded in full by its own workgroup before that
// workgroup's first barrier, and stored only after it.
#pragma once

#include "pdsp_packed.h"

namespace pdsp {

// p[0 ... 3] as 16-byte accesses (f32: one; f64: two); p 16-byte aligned
template <typename T>
__device__ __forceinline__ void ld_quad(const T *p, T (&v)[4]) {
  if constexpr (sizeof(T) == 4) {
    typedef float V4 __attribute__((ext_vector_type(4)));
    const V4 r = ld_stream(reinterpret_cast<const V4 *>(p));
    v[0] = r.x, v[1] = r.y, v[2] = r.z, v[3] = r.w;
  } else {
    typedef double V2 __attribute__((ext_vector_type(2)));
    const V2 a = ld_stream(reinterpret_cast<const V2 *>(p)), b = ld_stream(reinterpret_cast<const V2 *>(p) + 1);
    v[0] = a.x, v[1] = a.y, v[2] = b.x, v[3] = b.y;
  }
}
template <typename T>
__device__ __forceinline__ void st_quad(const T (&v)[4], T *p) {
  if constexpr (sizeof(T) == 4) {
    typedef float V4 __attribute__((ext_vector_type(4)));
    st_stream(V4{v[0], v[1], v[2], v[3]}, reinterpret_cast<V4 *>(p));
  } else {
    typedef double V2 __attribute__((ext_vector_type(2)));
    st_stream(V2{v[0], v[1]}, reinterpret_cast<V2 *>(p));
    st_stream(V2{v[2], v[3]}, reinterpret_cast<V2 *>(p) + 1);
  }
}

// x: `batch` rows at x_stride, y: rows at y_stride (y == x with the same stride allowed).  tw4: W_4N^k, k = 0 ... M.
template <typename T, int LOG2M, bool FAST>
__global__ void __launch_bounds__(kPackedWG<LOG2M>)
dct2_kernel(const T *x, const long long x_stride, T *y, const long long y_stride,
            const typename vec2<T>::type *__restrict__ tw, const typename vec2<T>::type *__restrict__ twr,
            const typename vec2<T>::type *__restrict__ tw4, const T g, const T g0, const long long batch) {
  using PR = PackedRow<T, LOG2M>;
  constexpr int E = PR::E, TP = PR::TP, M = PR::M, N = 2 * M;
  static_assert(TP * E / 2 == M / 2, "slots q < E/2 hold m < M/2");

  __shared__ cx<T> lds[PR::TR::LDS_ELEMS];
  const PR pr(lds, batch);
  const int tid = pr.tid;
  cx<T> *const lrow = pr.lrow;
  T *const lval = reinterpret_cast<T *>(lrow);  // N plain values (LROW >= M complex)
  const T *const xrow = x + (size_t)pr.row * (size_t)x_stride;

  PackedTwiddles<T, LOG2M> twd;
  twd.load(tw, twr, tid);
  load_order_fence();

  cx<T> z[E];
  if constexpr (FAST) {
    T v[E / 2][4];
    static_for<E / 2>([&](auto q) { ld_quad(xrow + 4 * (tid + TP * q), v[q]); });
    static_for<E / 2>([&](auto q) {
      const int m = tid + TP * q;
      lrow[lds_pad(m)] = cx<T>{v[q][0], v[q][2]};
      lrow[lds_pad(M - 1 - m)] = cx<T>{v[q][3], v[q][1]};
    });
    __syncthreads();
    fft_pass_readback<T, LOG2M, PR::LOG2E>(z, lrow, tid);
    __syncthreads();  // the first pass writes LDS again
  } else {
    static_for<E>([&](auto qc) {
      constexpr int q = qc;
      const int m = tid + TP * q;
      if constexpr (q < E / 2) {
        z[q] = cx<T>{ld_stream(xrow + 4 * (unsigned)m), ld_stream(xrow + 4 * (unsigned)m + 2)};
      } else {
        const unsigned mm = (unsigned)(M - 1 - m);
        z[q] = cx<T>{ld_stream(xrow + 4 * mm + 3), ld_stream(xrow + 4 * mm + 1)};
      }
    });
  }

  fft_passes<T, LOG2M, true, PR::LOG2E>(z, lrow, twd.twf, tid);  // Z in LDS, natural order
  __syncthreads();
  if constexpr (!FAST)
    if (!pr.live) return;  // no barrier below

  T *const yrow = y + (size_t)pr.row * (size_t)y_stride;
  const cx<T> *const w4 = reinterpret_cast<const cx<T> *>(tw4);
  T o[E / 2 + 1][4];  // y[k], y[N-k], y[M-k], y[M+k] of pair q (FAST: held across the barrier below)
  pr.for_each_pair([&](auto q, const int k) {
    const auto sp = pr.forward_split(k, (M - k) & (M - 1));
    const cx<T> w = twd.wk(q);  // W_N^k
    const cx<T> ca = cmul(sp.x(w), w4[k]);       // 2 V[k] W_4N^k
    const cx<T> cb = cmul(sp.xm(w), w4[M - k]);  // 2 V[M-k] W_4N^(M-k)
    o[q][0] = ca.x * (k == 0 ? g0 : g);
    o[q][1] = -ca.y * g;
    o[q][2] = cb.x * g;
    o[q][3] = -cb.y * g;
    if constexpr (!FAST) {
      yrow[k] = o[q][0];
      if (k != 0) yrow[N - k] = o[q][1];
      if (k != M / 2) {
        yrow[M - k] = o[q][2];
        if (k != 0) yrow[M + k] = o[q][3];
      }
    }
  });
  if constexpr (FAST) {
    __syncthreads();  // every Z read: the plain values take the row's LDS
    pr.for_each_pair([&](auto q, const int k) {
      lval[k] = o[q][0];
      if (k != 0) lval[N - k] = o[q][1];
      if (k != M / 2) {
        lval[M - k] = o[q][2];
        if (k != 0) lval[M + k] = o[q][3];
      }
    });
    __syncthreads();
    if (!pr.live) return;
    static_for<E / 2>([&](auto q) {
      const int c = 4 * (tid + TP * q);
      T v[4] = {lval[c], lval[c + 1], lval[c + 2], lval[c + 3]};
      st_quad(v, yrow + c);
    });
  }
}

// The DCT-III of the rows of x (scipy dct(type=3), g / g0 on the inputs), same layout rules as dct2_kernel.
template <typename T, int LOG2M, bool FAST>
__global__ void __launch_bounds__(kPackedWG<LOG2M>)
dct3_kernel(const T *x, const long long x_stride, T *y, const long long y_stride,
            const typename vec2<T>::type *__restrict__ tw, const typename vec2<T>::type *__restrict__ twr,
            const typename vec2<T>::type *__restrict__ tw4, const T g, const T g0, const long long batch) {
  using PR = PackedRow<T, LOG2M>;
  constexpr int E = PR::E, TP = PR::TP, M = PR::M, N = 2 * M;
  static_assert(TP * E / 2 == M / 2, "slots q < E/2 hold m < M/2");

  __shared__ cx<T> lds[PR::TR::LDS_ELEMS];
  const PR pr(lds, batch);
  const int tid = pr.tid;
  cx<T> *const lrow = pr.lrow;
  T *const lval = reinterpret_cast<T *>(lrow);  // N plain values (LROW >= M complex)
  const T *const xrow = x + (size_t)pr.row * (size_t)x_stride;

  PackedTwiddles<T, LOG2M> twd;
  twd.load_split(twr, tid);
  const cx<T> *const w4 = reinterpret_cast<const cx<T> *>(tw4);
  // inputs of pair q: x[k], x[N-k] (x[0] read for k = 0, then dropped), x[M-k], x[M+k]
  T a[E / 2 + 1][4];
  if constexpr (FAST) {
    T v[E / 2][4];
    static_for<E / 2>([&](auto q) { ld_quad(xrow + 4 * (tid + TP * q), v[q]); });
    static_for<E / 2>([&](auto q) {
      const int c = 4 * (tid + TP * q);
      lval[c] = v[q][0], lval[c + 1] = v[q][1], lval[c + 2] = v[q][2], lval[c + 3] = v[q][3];
    });
    __syncthreads();
    pr.for_each_pair([&](auto q, const int k) {
      a[q][0] = lval[k], a[q][1] = lval[(N - k) & (N - 1)], a[q][2] = lval[M - k], a[q][3] = lval[M + k];
    });
    __syncthreads();  // every plain value read: the split takes the row's LDS
  } else {
    pr.for_each_pair([&](auto q, const int k) {
      a[q][0] = ld_stream(xrow + (unsigned)k), a[q][1] = ld_stream(xrow + (unsigned)((N - k) & (N - 1)));
      a[q][2] = ld_stream(xrow + (unsigned)(M - k)), a[q][3] = ld_stream(xrow + (unsigned)(M + k));
    });
  }

  // V[k], V[M-k] and their inverse split
  pr.for_each_pair([&](auto q, const int k) {
    const int k2 = M - k;  // k = 0 pairs with the Nyquist bin M
    cx<T> va = cmul(cx<T>{a[q][0] * (k == 0 ? g0 : g), k == 0 ? T(0) : -a[q][1] * g}, conj(w4[k]));
    cx<T> vb = cmul(cx<T>{a[q][2] * g, -a[q][3] * g}, conj(w4[k2]));
    if (k == 0) va.y = vb.y = T(0);  // V[0] and V[M] are real
    pr.inverse_split(k, k2, va, vb, twd.wk(q));
  });
  twd.load_passes(tw, tid);
  cx<T> z[E];
  pr.second_transform(z, twd.twf);  // conj(v[2m] + i v[2m+1]) in slot q, m = tid + TP q

  T *const yrow = y + (size_t)pr.row * (size_t)y_stride;
  if constexpr (FAST) {
    __syncthreads();  // the last pass's read-back: the plain values take the row's LDS
    static_for<E>([&](auto qc) {
      constexpr int q = qc;
      const int m = tid + TP * q;
      if constexpr (q < E / 2) {
        lval[4 * m] = z[q].x, lval[4 * m + 2] = -z[q].y;
      } else {
        const int mm = M - 1 - m;
        lval[4 * mm + 3] = z[q].x, lval[4 * mm + 1] = -z[q].y;
      }
    });
    __syncthreads();
    if (!pr.live) return;
    static_for<E / 2>([&](auto q) {
      const int c = 4 * (tid + TP * q);
      T v[4] = {lval[c], lval[c + 1], lval[c + 2], lval[c + 3]};
      st_quad(v, yrow + c);
    });
  } else {
    if (!pr.live) return;
    static_for<E>([&](auto qc) {
      constexpr int q = qc;
      const int m = tid + TP * q;
      if constexpr (q < E / 2) {
        yrow[4 * (unsigned)m] = z[q].x, yrow[4 * (unsigned)m + 2] = -z[q].y;
      } else {
        const unsigned mm = (unsigned)(M - 1 - m);
        yrow[4 * mm + 3] = z[q].x, yrow[4 * mm + 1] = -z[q].y;
      }
    });
  }
}

}  // namespace pdsp

// pdsp_hilbert_kernel.h -- the Hilbert transform of real rows (scipy.signal.hilbert, even N) and what is read off
// the analytic signal a = x + i Hx, fused into one launch: samples in, Hx / a / |a| / arg a out, nothing in between
// leaves LDS.  It is the FIR kernel's data flow (pdsp_fir_kernel.h) with the filter spectrum replaced by a constant.
//
// One workgroup row owns one signal row of a plan of N = 2M points, `len` <= N samples zero-padded to N:
//   1. z[m] = x[2m] + i x[2m+1] (zero from len on), Z = FFT_M(z), on the packed-real tables;
//   2. 2 X[k], 2 X[M-k] by the forward split (pdsp_packed.h).  0 < k < M: both are positive frequencies, so
//      Y = -i X for both (a swap and a sign), times g = 1 / (2N) (a power of two: exact): Y / N.  The pair k = 0,
//      the DC and the Nyquist bin, is written as zeros;
//   3. the inverse split of Y / N into the row's LDS, and the second transform: Hx[2m] + i Hx[2m+1], conjugated, in
//      the registers that held z;
//   4. the row's own samples are loaded AGAIN (the same loads as step 1, by the same thread for the same slot, so a
//      thread re-reads only what it read before and, in place, reads it before its own stores; IMAG needs none),
//      and the epilogue writes, by `mode` (a launch-uniform switch: one kernel per size, precision and path),
//        ANALYTIC  x[n], Hx[n] interleaved (2N values per row; x is the loaded sample bit for bit),
//        IMAG      Hx[n],   ENVELOPE  |x[n] + i Hx[n]| (envelope_of: its range),   PHASE  atan2(Hx[n], x[n])
//        (N values per row).
// HBM traffic: one read (the second one is served by L2 / the memory-side cache when the row is still there, else
// it is a second read) and one write of N or 2N values per row.
// The three N-out modes may run exactly in place (y == x, same stride): a row is loaded in full by its own workgroup
// before that workgroup's first barrier, and each thread stores only to the samples it has just re-read.
#pragma once

#include "pdsp_packed.h"

namespace pdsp {

enum : int { kHilbertAnalytic = 0, kHilbertImag = 1, kHilbertEnvelope = 2, kHilbertPhase = 3 };

template <int V>
using int_k = std::integral_constant<int, V>;

// ENVELOPE, |a + i h|.
// f64 is range-safe, as mag(cx<double>) is (pdsp_fft_core.h), because the host forms restate
// np.abs(scipy.signal.hilbert(x)), a hypot: sqrt(a^2 + h^2) in f64 is Inf above |a| = 1.3e154 and 0 below 1.5e-162.  Both
// operands are scaled by 2^-e, e the exponent of the larger one (frexp: that one lands in [0.5, 1)), the squares are
// summed there, and the root is scaled back: three ldexp and one frexp_exp on top of the plain form, every one of them
// exact, so a row times 2^k gives the envelope times 2^k bit for bit over the whole range.  A smaller operand that
// underflows in the scaling or in its square is below half an ulp of the sum.  0 and non-finite operands have e = 0 and
// go through unscaled: 0 -> 0, Inf -> Inf, NaN -> NaN.  Cost: 1.3 - 4 % of the f64 ENVELOPE rate.
// f32 squares in f32 (no hypot), as mag(cx<float>) does: the envelope holds its bound for samples with
// 1.1e-19 <= |a| <= 1.8e19 (above: Inf; below, the squares are subnormal, then 0).  The scaled form above cost f32
// 5.7 - 7.7 % of its ENVELOPE rate at N = 1024 ... 16384, outside the tool's spread, and was not taken.
template <typename T>
__device__ __forceinline__ T envelope_of(const T a, const T h) {
  if constexpr (sizeof(T) == 8) {
    const int e = __builtin_amdgcn_frexp_exp(fmax(fabs(a), fabs(h)));
    const T as = ldexp(a, -e), hs = ldexp(h, -e);
    return ldexp(sqrt(fma(as, as, hs * hs)), e);
  } else {
    return sqrt(fma(a, a, h * h));
  }
}

// x: `batch` rows of `len` samples (1 <= len <= N) at x_stride; y: rows of N (ANALYTIC: 2N) values at y_stride.
// g = 1 / (2N).
//   FAST: len == N, x rows aligned to 2 sizeof(T) with even strides: 8- / 16-byte streaming loads; y rows aligned
//         to 2 sizeof(T) (ANALYTIC: to 16 bytes) with strides that keep that: pairs of outputs (ANALYTIC: x0, Hx0, x1,
//         Hx1) go out as 8- / 16-byte stores (non-temporal; f64 ANALYTIC: plain).  Otherwise clamped 32-bit loads with zero fill and scalar
//         stores.  (pdsp_host::hilbert_fast_path)
template <typename T, int LOG2M, bool FAST>
__global__ void __launch_bounds__(kPackedWG<LOG2M>)
hilbert_kernel(const T *xin, const int len, const long long x_stride, const int mode, T *yout,
               const long long y_stride, const typename vec2<T>::type *__restrict__ tw,
               const typename vec2<T>::type *__restrict__ twr, const T g, const long long batch) {
  using PR = PackedRow<T, LOG2M>;
  constexpr int E = PR::E, TP = PR::TP, M = PR::M;
  typedef T V2 __attribute__((ext_vector_type(2)));

  __shared__ cx<T> lds[PR::TR::LDS_ELEMS];
  const PR pr(lds, batch);
  const int tid = pr.tid;

  // the row's samples of slots Q0 ... Q0 + G - 1, slot q = x[2m] + i x[2m+1], m = tid + TP q: steps 1 and 4
  auto load_slots = [&](auto q0c, auto gc, cx<T>(&v)[E], const T *const xrow, const int len) {
    constexpr int Q0 = q0c, G = gc;
    if constexpr (FAST) {
      const cx<T> *const x2 = reinterpret_cast<const cx<T> *>(xrow);
      static_for<G>([&](auto i) { v[Q0 + i] = ld_stream(x2 + TP * (Q0 + i) + (unsigned)tid); });
    } else {
      // clamped loads + selects over the valid range [0, len), len >= 1
      static_for<G>([&](auto i) {
        const int n0 = 2 * (tid + TP * (Q0 + i)), n1 = n0 + 1;
        const int c0 = n0 < len ? n0 : len - 1, c1 = n1 < len ? n1 : len - 1;
        const T v0 = ld_stream(xrow + (unsigned)c0), v1 = ld_stream(xrow + (unsigned)c1);
        v[Q0 + i] = cx<T>{n0 < len ? v0 : T(0), n1 < len ? v1 : T(0)};
      });
    }
  };

  PackedTwiddles<T, LOG2M> twd;
  cx<T> x[E];
  load_slots(int_k<0>{}, int_k<E>{}, x, xin + (size_t)pr.row * (size_t)x_stride, len);
  twd.load(tw, twr, tid);  // the tables behind the row loads, as fir_overlap_save_kernel
  // The two paths promise bitwise equal results, so the arithmetic between the loads and the stores must compile the
  // same on both: the samples here and Hx below pass through an empty asm, which keeps the shape of the loads and of
  // the stores (packed or single, one mode's or another's) from reaching into the butterflies next to them.
  pin_regs<T, E>(x);

  fft_passes<T, LOG2M, true, PR::LOG2E>(x, pr.lrow, twd.twf, tid);  // Z in LDS, natural order
  __syncthreads();
  pr.for_each_pair([&](auto q, const int k) {
    const int k2 = (M - k) & (M - 1);
    const auto sp = pr.forward_split(k, k2);
    const cx<T> w = twd.wk(q);  // W_N^k
    cx<T> ya = mul_neg_i<T>(sp.x(w)) * g, yb = mul_neg_i<T>(sp.xm(w)) * g;  // -i X[k] / N, -i X[M-k] / N
    if (k == 0) ya = yb = cx<T>{T(0), T(0)};                                // Y[0] = Y[M] = 0
    pr.inverse_split(k, k2, ya, yb, w);
  });
  // f64 reads the table at every use in the second transform, as fir_overlap_save_kernel does (its comment)
  if constexpr (sizeof(T) == 8)
    pr.second_transform(x, TableTwiddles<T, LOG2M, PR::LOG2E>{reinterpret_cast<const cx<T> *>(tw)});
  else
    pr.second_transform(x, twd.twf);
  pin_regs<T, E>(x);

  if (!pr.live) return;
  // The second load must be one.  Left alone the compiler merges it with the first and the samples stay in E more
  // complex registers across both transforms: on the FAST path that costs f32 a workgroup per CU at N = 1024 ... 4096
  // and at N = 16384 (f64 still fits), on the general path it costs more and spills at f64 N = 16384 (DESIGN.md
  // 4.8).  The row stride (a kernel argument: uniform) passes through an empty asm, so the two address computations
  // are not the same value to the compiler; so does len, or the clamped offsets of the general path would stay in
  // registers instead.
  long long xs2 = x_stride;
  int len2 = len;
  asm volatile("" : "+s"(xs2), "+s"(len2));
  const T *const xrow = xin + (size_t)pr.row * (size_t)xs2;
  T *const yrow = yout + (size_t)pr.row * (size_t)y_stride;
  auto put2 = [&](const int n, const T v0, const T v1) {  // y[n], y[n+1], n even
    if constexpr (FAST) {
      st_stream(V2{v0, v1}, reinterpret_cast<V2 *>(yrow + (unsigned)n));
    } else {
      yrow[(unsigned)n] = v0;
      yrow[(unsigned)n + 1] = v1;
    }
  };
  // G slots at a time: all of them on the FAST path (E wide loads in flight); four on the general one, whose two
  // clamped loads per slot cost an offset register each on top of the E live slots of Hx
  constexpr int G = FAST ? E : 4;
  cx<T> s[E];
  static_for<E / G>([&](auto gi) {
    constexpr int Q0 = gi * G;
    if (mode != kHilbertImag) load_slots(int_k<Q0>{}, int_k<G>{}, s, xrow, len2);  // IMAG writes Hx alone
    if constexpr (!FAST) __builtin_amdgcn_sched_barrier(0);
    // slot q: samples n = 2m, 2m + 1 are s[q].x, s[q].y; Hx[n], Hx[n+1] are x[q].x, -x[q].y
    if (mode == kHilbertAnalytic) {
      static_for<G>([&](auto i) {
        constexpr int q = Q0 + i;
        const int n = 2 * (tid + TP * q);
        const T h0 = x[q].x, h1 = -x[q].y;
        if constexpr (FAST && sizeof(T) == 4) {
          typedef float V4 __attribute__((ext_vector_type(4)));
          st_stream(V4{s[q].x, h0, s[q].y, h1}, reinterpret_cast<V4 *>(yrow + 2 * (unsigned)n));
        } else {
          if constexpr (FAST) {
            // f64: two 16-byte stores per slot, 32 bytes apart from lane to lane, so each instruction fills half of
            // every cache line it touches.  As plain stores L2 combines them; as non-temporal ones they ran at 0.57 -
            // 0.78 of this rate
            *reinterpret_cast<V2 *>(yrow + 2 * (unsigned)n) = V2{s[q].x, h0};
            *reinterpret_cast<V2 *>(yrow + 2 * (unsigned)n + 2) = V2{s[q].y, h1};
          } else {
            put2(2 * n, s[q].x, h0);
            put2(2 * n + 2, s[q].y, h1);
          }
        }
      });
    } else if (mode == kHilbertImag) {
      static_for<G>([&](auto i) {
        constexpr int q = Q0 + i;
        put2(2 * (tid + TP * q), x[q].x, -x[q].y);
      });
    } else if (mode == kHilbertEnvelope) {
      static_for<G>([&](auto i) {
        constexpr int q = Q0 + i;
        const T h0 = x[q].x, h1 = -x[q].y;
        put2(2 * (tid + TP * q), envelope_of(s[q].x, h0), envelope_of(s[q].y, h1));
      });
    } else {
      static_for<G>([&](auto i) {
        constexpr int q = Q0 + i;
        const T h0 = x[q].x, h1 = -x[q].y;
        put2(2 * (tid + TP * q), atan2(h0, s[q].x), atan2(h1, s[q].y));
      });
    }
    if constexpr (!FAST) __builtin_amdgcn_sched_barrier(0);
  });
}

}  // namespace pdsp

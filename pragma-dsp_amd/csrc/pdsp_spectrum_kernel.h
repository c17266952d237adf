// pdsp_spectrum_kernel.h -- the fused bodies of spectrum(): window on load, packed transform, split, amplitudes out.
#pragma once

#include "pdsp_packed.h"
#include "pdsp_peaks.h"

namespace pdsp {

// Packed real frames for fft_split4_kernel: point m of the row is (x[2m], x[2m+1]) * (w[2m], w[2m+1]) of a
// frame of 2N samples, `stride` samples apart (16-byte aligned) -- the first pass of the packed-real
// spectrum path at N = 32768 (split_amp_rows_kernel undoes the packing).
// WIN: 0 rect, 1 window table (2N values), 2 / 3 two- / three-term cosine-sum window evaluated in registers
// (createWindow fused, fourier.ts:14-52): sample n = 8 (tid + 256 q) + e has, with f = 2 pi / (2N - 1) and
// cs(t) = (cos t, sin t),  cs(f n) = wb[tid] * wq[q] * we[e]  (wb[j] = cs(8 f j), wq[q] = cs(2048 f q),
// we[e] = cs(f e); f64-built), w = k0 + k1 c or k0 + c (k1 + k2 c), c = cos(f n).
template <typename T, int WIN>
struct LoadPackedFrames {
  const T *__restrict__ x;
  const T *__restrict__ win;
  long long stride;
  const float *wb, *wq, *we;
  float k0, k1, k2;
  static constexpr bool kPlanar = true;  // whole rows, vector loads
  static constexpr bool kHasIm = true;
  static constexpr bool kPacked = true;
  static constexpr int kWin = WIN;
};

// Loads are unconditional (clamped address + select): a per-element `if` around a
// load makes hipcc branch and drain vmcnt per element (cdna guide, section 5 item 4c).
template <typename T, bool HAS_WIN>
struct LoadFrameWindowed {  // buildFrame + applyWindow, spectrum.ts:36-43, :116-119
  const T *__restrict__ x;
  const T *__restrict__ win;  // N values when HAS_WIN (rect otherwise)
  long long frame_len;        // 1 <= samples used per row <= N; the rest reads as zero
  long long stride;
  __device__ __forceinline__ cx<T> operator()(long long row, int off, int lane) const {
    const int i = off + lane;
    const int last = (int)frame_len - 1;
    T v = ld_stream(x + (size_t)row * (size_t)stride + (unsigned)(i < last ? i : last));
    v = i <= last ? v : T(0);
    if constexpr (HAS_WIN) v *= win[i];
    return cx<T>{v, T(0)};
  }
};

template <typename T>
struct StoreAmplitude {  // magnitude + scaleAmplitude{One,Two}Sided [+ phase]
  T *__restrict__ amp;
  T *__restrict__ ph;  // may be null
  int bins;            // N/2+1 or N
  int nyq;             // N/2 for one-sided (that bin is not doubled), -1 for two-sided
  T s_edge;            // 1/N
  T s_mid;             // 2/N one-sided, 1/N two-sided
  __device__ __forceinline__ void operator()(long long row, int off, int lane, cx<T> v) const {
    const int i = off + lane;
    if (i < bins) {
      const size_t o = (size_t)row * (size_t)bins;
      st_stream(mag(v) * ((i == 0 || i == nyq) ? s_edge : s_mid), amp + o + (unsigned)i);
      if (ph) st_stream(T(atan2(v.y, v.x)), ph + o + (unsigned)i);
    }
  }
};

// Tables of a FUSED cosine-sum window (createWindow of src/xform/fourier.ts:14-52 evaluated in the kernel
// instead of read from an N-value table): a thread's sample indices are n = (2 tid + e) + 2 TP q (+ N/2 in
// the N = 16384 kernel), so cos(f n), f = 2 pi / (N - 1), is one angle addition from a per-thread base and a
// per-q constant; w = k0 + c (k1 + k2 c) with (k0, k1, k2) = (a0 - a2, -a1, 2 a2)  [cos 2x = 2 c^2 - 1].
struct WinFused {
  const float *base;  // [TP][4]: cos, sin of f*(2 tid), cos, sin of f*(2 tid + 1)
  const float *step;  // [16][2]: cos, sin of f*2 TP q (q < 16); N = 16384 kernel: [32][2], the second half for + N/2
  float k0, k1, k2;
  // the coefficients above already carry the amplitude scale s_mid / 2 (a power of two: exact), so the
  // Hermitian split multiplies by nothing; edge_ratio = s_edge / s_mid fixes up the two bins that are
  // not doubled (DC, Nyquist)
  float edge_ratio;
};

// Fused body of spectrum() for real frames, one frame per row, via the packed-real
// identity: z[m] = x[2m] + i*x[2m+1] (a plain 2-wide view of the windowed frame),
// Z = FFT_M(z) with M = N/2, then for each pair (k, M-k)
//     E = (Z[k] + conj Z[M-k]) / 2,  O = (Z[k] - conj Z[M-k]) / (2i),  t = W_N^k * O,
//     X[k] = E + t,   X[M-k] = conj(E - t),          (k = 0 also yields X[M] = Nyquist)
// and only |X| (scaled as scaleAmplitude{One,Two}Sided, spectrum.ts:45-72) and
// optionally atan2 leave the chip.  Half the butterflies, half the LDS and half the
// loads per thread of running the complex kernel on (x, 0).
//   LOG2M = log2(N/2) >= 5.   twr[k] = e^{-2*pi*i*k/N}, 0 <= k <= M/2.
//   FAST: whole, 8-byte aligned frames (frame_len == N, even stride), one-sided
//         amplitude only -- the config-4 shape: 8-byte loads, no selects, and the phase /
//         mirror code stays out of the (VALU-issue bound) instruction stream.
//   !FAST: any frame_len >= 1 / alignment (scalar clamped loads + selects), phase and
//         two-sided output at run time.
//   PEAK: also reduce each frame to its SpectrumPeak (findPeak fused; `amp` may then be
//         null = peaks-only output, 16 B per frame instead of 2*(N/2+1) B).
//   WIN: 0 = rect, 1 = window table (N values), 2 / 3 = two- / three-term cosine-sum window FUSED (WinFused;
//        FAST f32 only): no table traffic, 3-4 packed instructions per pair of samples.
template <typename T, int LOG2M, bool FAST, int WIN, bool PEAK>
__global__ void __launch_bounds__(kPackedWG<LOG2M>)
spectrum_packed_kernel(const T *__restrict__ frames, const T *__restrict__ win, const WinFused wf, const long long frame_len,
                       const long long stride, const typename vec2<T>::type *__restrict__ tw,
                       const typename vec2<T>::type *__restrict__ twr, T *__restrict__ amp,
                       T *__restrict__ ph, const int two_sided, const T s_edge, const T s_mid,
                       PeakRec *__restrict__ peaks, const T freq_scale, const long long batch) {
  using PR = PackedRow<T, LOG2M>;
  constexpr int E = PR::E, TP = PR::TP, M = PR::M;
  constexpr bool HAS_WIN = WIN == 1;
  static_assert(WIN <= 1 || (FAST && sizeof(T) == 4), "fused windows: whole f32 frames");
  // adjacent-bin 8-byte non-temporal stores pay when a wave's stores cover whole cache lines of one row
  // (TP >= 32: N >= 1024).  Below that a wave spans many short rows and each lane's 8 / 16 bytes would be
  // a partial-line streaming write: measured 1.8 -> 0.8 TB/s at N = 64 (f32, staged path off) and
  // 36 -> 22 % in f64 -- those sizes keep round 1's split (dword stores that L2 merges).
  constexpr bool kAdj = FAST && TP >= 32;
  typedef T V4 __attribute__((ext_vector_type(4)));

  __shared__ cx<T> lds[PR::TR::LDS_ELEMS];
  const PR pr(lds, batch);
  const int tid = pr.tid;
  // pr.lrow, spelled on the array itself: taken from the constructed row it costs the general variants 1-4 VGPRs
  cx<T> *const lrow = lds + (int)(threadIdx.x / TP) * PR::TR::LROW;

  // buildFrame + applyWindow (spectrum.ts:36-43, :116-119) on load; m = tid + TP*q
  const T *const xrow = frames + (size_t)pr.row * (size_t)stride;
  cx<T> x[E];
  // tables first: twiddle bases, the split twiddle, the thread's window values
  PackedTwiddles<T, LOG2M> twd;
  V4 tb = V4{T(0), T(0), T(0), T(0)};  // kAdj: (W_N^(2 tid), W_N^(2 tid + 1)), the split's two bases
  V4 wb4 = V4{T(0), T(0), T(0), T(0)};  // fused window: the thread's base (cos, sin) pairs
  cx<T> wv[HAS_WIN ? E : 1];
  twd.load_passes(tw, tid);
  if constexpr (kAdj) tb = reinterpret_cast<const V4 *>(twr)[(unsigned)tid];
  else twd.load_split(twr, tid);
  if constexpr (WIN >= 2) wb4 = reinterpret_cast<const V4 *>(wf.base)[(unsigned)tid];
  if constexpr (HAS_WIN && FAST) {
    const cx<T> *const w2 = reinterpret_cast<const cx<T> *>(win);
    static_for<E>([&](auto q) { wv[q] = (w2 + TP * q)[(unsigned)tid]; });
  } else if constexpr (HAS_WIN) {
    // the general variant takes a window at ANY alignment (a view one value into a tensor): two scalar loads
    static_for<E>([&](auto q) { wv[q] = cx<T>{(win + 2 * TP * q)[2 * (unsigned)tid], (win + 2 * TP * q + 1)[2 * (unsigned)tid]}; });
  }
  load_order_fence();
  // (Buffer-form addressing -- one descriptor per row, scalar q offsets -- gains 4-5 % on the N = 16384
  // kernel, where it removes ~100 address instructions; here, A/B with tools/sweep.py, it measured +-0 at
  // N = 2048 / 8192 and -2 % at 4096, so the flat form stays.)
  if constexpr (FAST) {
    const cx<T> *const x2 = reinterpret_cast<const cx<T> *>(xrow);
    static_for<E>([&](auto q) { x[q] = ld_stream(x2 + TP * q + (unsigned)tid); });
  } else {
    // unconditional clamped loads + selects (no per-element branches); 1 <= frame_len <= N
    const int flen = (int)frame_len;
    static_for<E>([&](auto q) {
      const int i0 = 2 * (tid + TP * q);
      const int c0 = i0 < flen - 1 ? i0 : flen - 1, c1 = i0 + 1 < flen - 1 ? i0 + 1 : flen - 1;
      const T v0 = ld_stream(xrow + (unsigned)c0), v1 = ld_stream(xrow + (unsigned)c1);
      x[q] = cx<T>{i0 < flen ? v0 : T(0), i0 + 1 < flen ? v1 : T(0)};
    });
  }
  PDSP_STAMP_INIT();
  load_order_fence();
  if constexpr (HAS_WIN) static_for<E>([&](auto q) { x[q] = x[q] * wv[q]; });
  if constexpr (WIN >= 2) {
    static_assert(WIN < 2 || kAdj, "the fused windows' pre-scaled frames are split by the adjacent-bin code");
    const cx<T> cb{wb4.x, wb4.z}, sb{wb4.y, wb4.w};  // (e = 0, e = 1)
    const T k0 = wf.k0, k1 = wf.k1, k2 = wf.k2;        // pre-scaled by s_mid / 2 on the host (WinFused)
    const cx<T> kc = cb * k1, ks = sb * k1;             // two-term form: w = k0 + kc cos_q - ks sin_q
    static_for<E>([&](auto qc) {
      constexpr int q = qc;
      const T cq = wf.step[2 * q], sq = wf.step[2 * q + 1];  // wave-uniform: scalar loads
      if constexpr (WIN == 3) {
        const cx<T> c = cb * cq - sb * sq;                   // cos(f n), n = 2 (tid + TP q) + e
        x[q] = x[q] * (k0 + c * (k1 + k2 * c));
      } else {
        x[q] = x[q] * ((k0 + kc * cq) - ks * sq);
      }
    });
  }
  // The adjacent-bin split takes a frame PRE-SCALED by g = s_mid / 2 (a power of two: exact) and multiplies by
  // nothing: the fused windows carry g in their coefficients (WinFused); the rect and table variants multiply here --
  // one packed multiply per pair of samples instead of four per pair of bins.  edge = s_edge / s_mid fixes up DC and
  // Nyquist, which are not doubled.
  const T edge = WIN >= 2 ? T(wf.edge_ratio) : s_edge / s_mid;
  if constexpr (kAdj && WIN <= 1) {
    const T g = T(0.5) * s_mid;
    static_for<E>([&](auto q) { x[q] = x[q] * g; });
  }
#ifdef PDSP_STAMPS
  pin_regs<T, E>(x);  // land the frame + window here
#endif
  PDSP_STAMP(0);  // frame + window loads

  fft_passes<T, LOG2M, true, PR::LOG2E>(x, lrow, twd.twf, tid);
  __syncthreads();
  PDSP_STAMP(1);  // all passes (detail in slots 8..)

  const int bins = (!FAST && two_sided) ? 2 * M : M + 1;
  const bool store_amp = pr.live && (!PEAK || amp != nullptr);
  T *const arow = amp + (size_t)pr.row * (size_t)bins;
  T *const prow = (!FAST && ph) ? ph + (size_t)pr.row * (size_t)bins : nullptr;
  // (the ordered runs of spectrum_dif16k_kernel -- PeakBest::consider_ascending / _descending -- measured +-0 at
  // N = 4096 and -2.3 % at N = 1024 here, where a thread owns 16 bins, not 32: the order-independent rule stays)
  PeakBest<T> best{T(0), 0, cx<T>{T(0), T(0)}};
  T dc_amp = T(0);
  cx<T> dc_x{T(0), T(0)};
  if constexpr (kAdj) {
    // FAST split, round 2: a thread takes ADJACENT bins -- k0 = 2 (tid + TP q'), k1 = k0 + 1, q' < 4 -- so
    // that its outputs are the pairs (k0, k0+1) and (M-k0-1, M-k0): 8-byte non-temporal stores (the shape
    // that measured 6.0 vs 5.6 TB/s on the N = 16384 load / store skeleton, tools/kbench2) instead of
    // dword stores in two directions.  W_N^(k0 + e) = twr[2 tid + e] * W_16^q'  (N = 32 TP).
    typedef T V2 __attribute__((ext_vector_type(2)));
    const cx<T> tw0{tb.x, tb.y}, tw1{tb.z, tb.w};
    static_for<4>([&](auto qc) {
      constexpr int q = qc;
      const int k0 = 2 * (tid + TP * q);  // even, < M/2
      const cx<T> z0 = lrow[lds_pad(k0)], z1 = lrow[lds_pad(k0) + 1];          // k0 % 16 <= 14: same block of 16
      const cx<T> zp0 = lrow[lds_pad((M - k0) & (M - 1))], zp1 = lrow[lds_pad(M - k0 - 1)];
      const cx<T> w0 = mul_w32<T, 2 * q>(tw0), w1 = mul_w32<T, 2 * q>(tw1);
      // the frame came in pre-scaled by s_mid / 2: no multiplies here; DC and Nyquist (k0 = 0: not doubled) are
      // fixed up on xa0 / xb0 below
      const cx<T> e0 = z0 + conj(zp0), p0 = cmul(z0 - conj(zp0), w0);
      const cx<T> e1 = z1 + conj(zp1), p1 = cmul(z1 - conj(zp1), w1);
      cx<T> xa0 = add_mul_neg_i(e0, p0), xb0 = conj(add_mul_pos_i(e0, p0));        // X[k0], X[M - k0]
      const cx<T> xa1 = add_mul_neg_i(e1, p1), xb1 = conj(add_mul_pos_i(e1, p1));  // X[k0 + 1], X[M - k0 - 1]
      if constexpr (q == 0) {
        const T r = tid == 0 ? edge : T(1);  // k0 = 0 lives in thread 0's first pair
        xa0 = xa0 * r;
        xb0 = xb0 * r;
      }
      const T ma0 = mag(xa0), mb0 = mag(xb0), ma1 = mag(xa1), mb1 = mag(xb1);
      if constexpr (PEAK) {
        if (k0 == 0) {
          dc_amp = ma0;
          dc_x = xa0;
        } else {
          best.consider(ma0, k0, xa0);
        }
        best.consider(ma1, k0 + 1, xa1);
        best.consider(mb1, M - k0 - 1, xb1);
        best.consider(mb0, M - k0, xb0);
      }
      if (store_amp) {
        __builtin_nontemporal_store(V2{ma0, ma1}, reinterpret_cast<V2 *>(arow + (unsigned)k0));
        __builtin_nontemporal_store(V2{mb1, mb0}, reinterpret_cast<V2 *>(arow + (unsigned)(M - k0 - 1)));
      }
    });
    if (tid == 0) {  // the middle bin M/2 pairs with itself: X[M/2] = conj(Z[M/2]) scaled
      const cx<T> xm = conj(lrow[lds_pad(M / 2)]) * T(2);  // the pre-scaled frame carries s_mid / 2; one value, not a sum
      const T mm = mag(xm);
      if constexpr (PEAK) best.consider(mm, M / 2, xm);
      if (store_amp) arow[(unsigned)(M / 2)] = mm;
    }
  }
  // pairs k = tid + TP*q, q < E/2 (k < M/2); k = M/2 is one more pair for tid == 0
  const auto pairs = pr.pairs(lrow);
  static_for<kAdj ? 0 : E / 2 + 1>([&](auto qc) {
    constexpr int q = qc;
    if (q < E / 2 || tid == 0) {
      const int k = tid + TP * q, k2 = M - k;
      const auto sp = pairs.forward_split(qc, k, k2 & (M - 1));
      const cx<T> w = twd.wk(qc);                          // W_N^k
      // the amplitude scale rides on the 1/2 of the split; bins 0 (DC, from k = 0) and M (Nyquist, the
      // partner of k = 0) are not doubled.  A positive scale leaves the phases untouched.
      const T h = T(0.5) * ((k == 0) ? s_edge : s_mid);
      const cx<T> e = sp.s() * h;                          // scaled E
      const cx<T> p = sp.p(w) * h;                         // scaled i * O * W, O = (Z - conj Zp)/(2i)
      const cx<T> xa = add_mul_neg_i(e, p);                // scaled X[k] = E + W*O
      const cx<T> xb = conj(add_mul_pos_i(e, p));          // scaled X[M-k] = conj(E - W*O)
      const T ma = mag(xa), mb = mag(xb);
      if constexpr (PEAK) {
        // the mirrored two-sided bins N-k carry identical values at larger indices, so
        // the strict-'>' search never selects them: bins 1..M decide
        if (k == 0) {
          dc_amp = ma;
          dc_x = xa;
        } else {
          best.consider(ma, k, xa);
        }
        if (k2 != k) best.consider(mb, k2, xb);
      }
      if (store_amp) {
        arow[(unsigned)k] = ma;
        if (k2 != k) arow[(unsigned)k2] = mb;
        if constexpr (!FAST) {
          if (two_sided && k != 0) {  // X[N-k] = conj X[k]
            arow[(unsigned)(2 * M - k)] = ma;
            if (k2 != k) arow[(unsigned)(2 * M - k2)] = mb;
          }
          if (prow) {
            prow[(unsigned)k] = T(atan2(xa.y, xa.x));
            if (k2 != k) prow[(unsigned)k2] = T(atan2(xb.y, xb.x));
            if (two_sided && k != 0) {
              prow[(unsigned)(2 * M - k)] = T(atan2(-xa.y, xa.x));
              if (k2 != k) prow[(unsigned)(2 * M - k2)] = T(atan2(-xb.y, xb.x));
            }
          }
        }
      }
    }
  });

  PDSP_STAMP(2);  // Hermitian split + stores issued
  if constexpr (PEAK) {
    // row-wide arg-max: butterflies inside the wave, then one LDS hop across the row's waves
    constexpr int WSPAN = TP < 64 ? TP : 64;
    static_for<ilog2(WSPAN)>([&](auto sc) {
      constexpr int off = WSPAN >> (sc + 1);
      const PeakBest<T> o{__shfl_xor(best.v, off, 64), __shfl_xor(best.i, off, 64),
                          cx<T>{__shfl_xor(best.x.x, off, 64), __shfl_xor(best.x.y, off, 64)}};
      best.consider(o.v, o.i, o.x);
    });
    if constexpr (TP > 64) {
      constexpr int WAVES = TP / 64;  // waves per row; ROWS == 1 or WG/TP rows of WAVES waves
      __shared__ T pk_v[PR::TR::WG / 64];
      __shared__ int pk_i[PR::TR::WG / 64];
      __shared__ cx<T> pk_x[PR::TR::WG / 64];
      const int wave = (int)threadIdx.x / 64;
      if ((threadIdx.x & 63) == 0) {
        pk_v[wave] = best.v;
        pk_i[wave] = best.i;
        pk_x[wave] = best.x;
      }
      __syncthreads();
      if (tid == 0) {
        static_for<WAVES - 1>([&](auto wc) {
          const int w = (int)(threadIdx.x / TP) * WAVES + wc + 1;  // rloc * WAVES: the row's first wave
          best.consider(pk_v[w], pk_i[w], pk_x[w]);
        });
      }
    }
    if (pr.live && tid == 0) store_peak_fused(peaks, pr.row, best, dc_amp, dc_x, freq_scale);
  }
}

// Fused spectrum for small frames (64 <= N <= 512), the staged counterpart of
// spectrum_packed_kernel's FAST variant: whole contiguous 16-byte aligned frames, one-sided
// amplitude.  The workgroup's 4096/M frames are one contiguous 8192-float chunk: staged in with
// 16-byte loads (window applied on the way), transformed and split as in the packed kernel, and
// the amplitude rows -- N/2+1 floats each, so no row starts aligned -- are staged out through an
// LDS row buffer and leave as one linear, fully coalesced stream.  Measured (tools/sweep.py):
// N = 64: 1.9 -> 5.6 TB/s, 128: 2.8 -> 5.9, 256: 3.9 -> 5.7, 512: 4.9 -> 5.4; from N = 1024 up the
// extra LDS round trip and workgroup-wide barrier cost more than they save (4.6 vs 5.0 TB/s).
template <typename T, int LOG2M, bool HAS_WIN>
__global__ void __launch_bounds__(256)
spectrum_staged_kernel(const T *__restrict__ frames, const T *__restrict__ win,
                       const typename vec2<T>::type *__restrict__ tw, const typename vec2<T>::type *__restrict__ twr,
                       T *__restrict__ amp, const T s_edge, const T s_mid, const long long batch) {
  using TR = FftTraits<LOG2M>;
  constexpr int M = TR::N, N = 2 * M, E = TR::E, TP = TR::TP, ROWS = TR::ROWS, WG = 256;
  static_assert(TR::WG == WG && TR::NP > 1 && LOG2M >= 5 && LOG2M <= 8, "staged spectrum: 64 <= N <= 512");
  constexpr int IN_FLOATS = ROWS * N;         // 8192
  constexpr int OUT_FLOATS = ROWS * (M + 1);  // 4096 + ROWS
  typedef T V4 __attribute__((ext_vector_type(4)));
  __shared__ cx<T> lds[TR::LDS_ELEMS];
  __shared__ T ampbuf[OUT_FLOATS];

  const int t = (int)threadIdx.x;
  const int tid = t % TP, rloc = t / TP;
  cx<T> *const lrow = lds + rloc * TR::LROW;
  const size_t in_base = (size_t)blockIdx.x * IN_FLOATS, in_limit = (size_t)batch * N;

  // frames -> LDS: float 4j.. of the chunk are points m, m+1 (m even) of local row (4j)/N
  static_for<IN_FLOATS / 4 / WG>([&](auto ic) {
    const int p = 4 * (t + WG * ic);
    size_t g = in_base + (size_t)p;
    g = g + 4 <= in_limit ? g : in_limit - 4;  // tail workgroup: re-read valid floats; dead rows never store
    V4 v = ld_stream(reinterpret_cast<const V4 *>(frames + g));
    if constexpr (HAS_WIN) v = v * reinterpret_cast<const V4 *>(win)[(p % N) / 4];  // applyWindow
    cx<T> *const d = lds + (p / N) * TR::LROW + lds_pad((p % N) / 2);
    d[0] = cx<T>{v.x, v.y};
    d[1] = cx<T>{v.z, v.w};
  });
  __syncthreads();
  cx<T> x[E];
  static_for<E>([&](auto q) { x[q] = lrow[lds_pad(tid + TP * q)]; });
  __syncthreads();  // the first pass scatters into the same buffer

  PackedTwiddles<T, LOG2M, true> twd;  // register bases at every size (TP = 2 ... 16)
  twd.load(tw, twr, tid);
  fft_passes<T, LOG2M, true>(x, lrow, twd.twf, tid);
  __syncthreads();

  // Hermitian split (see spectrum_packed_kernel) into the LDS row buffer
  T *const arow = ampbuf + rloc * (M + 1);
  static_for<E / 2 + 1>([&](auto qc) {
    constexpr int q = qc;
    if (q < E / 2 || tid == 0) {
      const int k = tid + TP * q, k2 = M - k;
      const typename PackedRow<T, LOG2M>::Split sp{lrow[lds_pad(k)], lrow[lds_pad(k2 & (M - 1))]};
      const cx<T> w = twd.wk(qc);  // W_N^k
      // the amplitude scale rides on the 1/2 of the split: DC and Nyquist (k = 0) are not doubled
      const T h = T(0.5) * ((k == 0) ? s_edge : s_mid);
      const cx<T> e = sp.s() * h;
      const cx<T> p = sp.p(w) * h;  // i * W * O
      arow[k] = mag(add_mul_neg_i(e, p));
      if (k2 != k) arow[k2] = mag(add_mul_pos_i(e, p));  // |conj(.)| = |.|
    }
  });
  __syncthreads();

  const size_t out_base = (size_t)blockIdx.x * OUT_FLOATS, out_limit = (size_t)batch * (M + 1);
  static_for<(OUT_FLOATS + WG - 1) / WG>([&](auto ic) {
    const int i = t + WG * ic;
    if (i < OUT_FLOATS && out_base + (size_t)i < out_limit) amp[out_base + (size_t)i] = ampbuf[i];
  });
}

#ifndef PDSP_DIF16K_WAVES
#define PDSP_DIF16K_WAVES 3  // three workgroups per CU (~160 VGPRs fit the 168 budget)
#endif
// spectrum() body for N = 16384 real frames, the config-4 shape (whole 8-byte-aligned frames, one-sided
// amplitude, optional fused findPeak), cut so that THREE frames fit a CU: the packed transform
// Z = FFT_8192(z), z[m] = x[2m] + i*x[2m+1], is one radix-2 decimation-in-FREQUENCY step over two
// 4096-point transforms that the same 256 threads run back to back through one 4096-point LDS buffer
// (spectrum_packed_kernel<13> needs 69.6 KB of LDS per frame and 5 full-size LDS round trips; here
// 34.8 KB and 2.5).  Round 1 made the cut by decimation in TIME (16-byte loads, Z[k] / Z[k+4096] in
// registers, dword stores): same arithmetic, 4.65-5.05 TB/s by box; this cut, with the fused Hann window,
// buffer addressing and the scale folded into the window: 5.6-6.0.
//   u[m] = z[m] + z[m+4096],  v[m] = (z[m] - z[m+4096]) * W_8192^m,   m < 4096;
//   U = FFT_4096(u) = the even bins Z[2k],  V = FFT_4096(v) = the odd bins Z[2k+1].
// The radix-2 step sits in front of the sub-transforms, which shapes the memory accesses at both ends
// (tools/kbench2: the load / store skeleton of this shape runs at 5.9-6.0 TB/s against 5.5-5.6 for the
// decimation-in-time shape, on a part whose 2:1 read:write copy tops out at 6.1-6.3):
//   * a thread needs z[m] and z[m+4096], m = tid + 256q: plain 8-byte loads at unit stride across the
//     lanes (32 per thread) instead of 16-byte loads that drag two sub-sequences along;
//   * the Hermitian split pairs Z[j] with Z[8192-j]: even with even, odd with odd, so thread tid ends up
//     owning bins (2k, 2k+1) and their mirrors (8191-2k, 8192-2k), k = tid + 256q, q < 8 -- ADJACENT
//     bins: 16 non-temporal 8-byte stores per thread instead of 33 dword stores in two directions.
//     (Non-temporal matters: plain 8-byte stores measured 5.4, non-temporal 6.0 TB/s; dword stores are
//     the other way round because a wave's 256 unaligned bytes are completed by its neighbours in L2.)
//   * partners: U[4096-k] and V[4095-k] live in the upper eight registers of thread 256-tid / 255-tid:
//     every thread parks its upper eight U and V values in LDS (32 KB, unit stride, no padding needed)
//     and reads eight of each back, lanes reversed.
// 34.8 KB of LDS (the sub-transforms' exchange buffer), three workgroups per CU.
//   tw12 = radix table of the 4096-point transform; twr[k] = W_16384^k, k <= 4096.
//   WIN: 0 = rect; 1 = window table (N values, 8-byte loads: 64 KB of L2 reads per frame -- measured
//   11 % of the kernel's time, 5.32 vs 5.97 TB/s); 2 / 3 = createWindow FUSED (fourier.ts:14-52): the
//   reference's windows are cosine sums a0 - a1 cos(f n) + a2 cos(2 f n), f = 2 pi / (N - 1), and a
//   thread's sample indices are n = (2 tid + e) + 512 q (+ 8192), so cos(f n) is one angle addition from
//   a per-thread base (one 16-byte load: cos / sin of f (2 tid + e), e = 0, 1) and a per-q constant
//   (wave-uniform: scalar loads): 3-4 packed instructions per pair of samples and no table traffic.
//   (WinFused above; values agree with the f64-built, f32-rounded table to ~2e-7 absolute.)
template <typename T, int WIN, bool PEAK>
__global__ void __launch_bounds__(256, PDSP_DIF16K_WAVES)
spectrum_dif16k_kernel(const T *__restrict__ frames, const T *__restrict__ win, const WinFused wf, const long long stride,
                       const typename vec2<T>::type *__restrict__ tw12,
                       const typename vec2<T>::type *__restrict__ twr, T *__restrict__ amp, const T s_edge,
                       const T s_mid, PeakRec *__restrict__ peaks, const T freq_scale, const long long batch) {
  constexpr bool HAS_WIN = WIN == 1;
  static_assert(sizeof(T) == 4, "f32 only: f64 frames of N = 16384 run on spectrum_packed_kernel<double, 13>");
  using TR = FftTraits<12>;
  constexpr int E = 16, TP = 256, H = 4096, M = 8192, Q = 2048;
  typedef T V4 __attribute__((ext_vector_type(4)));
  __shared__ cx<T> lds[TR::LROW];

  const int tid = (int)threadIdx.x;
  const long long row = uniform_row<TP>((long long)blockIdx.x);
  if (row >= batch) return;
  const cx<T> *const tw = reinterpret_cast<const cx<T> *>(tw12);

  // tables first: twiddle bases, the two split bases, the thread's window values
  RegTwiddles<T, 12> twf;
  twf.load(tw, tid);
  // (W_16384^(2 tid), W_16384^(2 tid + 1)) in one 16-byte load: the first is W_8192^tid, base of the
  // decimation twiddle W_8192^(tid+256q) = wc0 * W32^q AND of the even bins' split twiddle W_16384^(2k);
  // the second is the base of the odd bins' W_16384^(2k+1) = ws1 * W32^q
  const V4 wcs = reinterpret_cast<const V4 *>(twr)[(unsigned)tid];
  const cx<T> wc0{wcs.x, wcs.y}, ws1{wcs.z, wcs.w};
  cx<T> wlo[HAS_WIN ? E : 1], whi[HAS_WIN ? E : 1];
  if constexpr (HAS_WIN) {
    const cx<T> *const w2 = reinterpret_cast<const cx<T> *>(win);
    static_for<E>([&](auto q) {
      wlo[q] = (w2 + TP * q)[(unsigned)tid];
      whi[q] = (w2 + H + TP * q)[(unsigned)tid];
    });
  }
  V4 wb4 = V4{T(0), T(0), T(0), T(0)};
  if constexpr (WIN >= 2) wb4 = reinterpret_cast<const V4 *>(wf.base)[(unsigned)tid];
  load_order_fence();

  // z[m], z[m + 4096], m = tid + 256q: 8-byte non-temporal loads, unit stride across the lanes.
  // One buffer descriptor for the frame, ONE per-lane offset register (8 tid) and the 2048 q (+ 32768) part as a
  // scalar offset -- with flat addresses hipcc built a 64-bit vector address per load (v_add_co / s_nop / v_addc:
  // the q offsets exceed the 13-bit immediate), ~100 of the kernel's ~1300 issue slots, on a kernel whose vector
  // issue is its busiest resource.
  const cx<T> *const z2 = reinterpret_cast<const cx<T> *>(frames + (size_t)row * (size_t)stride);
  cx<T> a[E], b[E];
  const __amdgpu_buffer_rsrc_t rs =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<cx<T> *>(z2), 0, 2 * M * (int)sizeof(T), 0x00020000);
  const int vo = tid * 8;
  static_for<E>([&](auto q) {
    a[q] = __builtin_bit_cast(cx<T>, __builtin_amdgcn_raw_buffer_load_b64(rs, vo, 2048 * q, 2 /* nt */));
    b[q] = __builtin_bit_cast(cx<T>, __builtin_amdgcn_raw_buffer_load_b64(rs, vo, 32768 + 2048 * q, 2));
  });
  load_order_fence();
  // Every variant hands the sub-transforms a frame PRE-SCALED by g = s_mid / 2 (a power of two: exact), so that the
  // Hermitian split multiplies by nothing: the fused windows carry g in their coefficients (WinFused), the table
  // and rect variants multiply here (one packed multiply per pair of samples, against four per bin pair in the
  // split).  DC and Nyquist, which are not doubled, get edge = s_edge / s_mid on their two values.
  const T edge = WIN >= 2 ? T(wf.edge_ratio) : s_edge / s_mid;
  if constexpr (WIN <= 1) {
    const T g = T(0.5) * s_mid;
    static_for<E>([&](auto q) {
      if constexpr (HAS_WIN) {
        a[q] = a[q] * (wlo[q] * g);
        b[q] = b[q] * (whi[q] * g);
      } else {
        a[q] = a[q] * g;
        b[q] = b[q] * g;
      }
    });
  }
  if constexpr (WIN >= 2) {
    const cx<T> cb{wb4.x, wb4.z}, sb{wb4.y, wb4.w};  // (e = 0, e = 1)
    const T k0 = wf.k0, k1 = wf.k1, k2 = wf.k2;        // pre-scaled by s_mid / 2 on the host (WinFused)
    const cx<T> kc = cb * k1, ks = sb * k1;             // two-term form: w = k0 + kc cos_q - ks sin_q
    static_for<E>([&](auto qc) {
      constexpr int q = qc;
      const T cl = wf.step[2 * q], sl = wf.step[2 * q + 1], ch = wf.step[32 + 2 * q], sh = wf.step[32 + 2 * q + 1];
      if constexpr (WIN == 3) {
        const cx<T> c_lo = cb * cl - sb * sl, c_hi = cb * ch - sb * sh;  // cos(f n), n = 2m + e and + 8192
        a[q] = a[q] * (k0 + c_lo * (k1 + k2 * c_lo));
        b[q] = b[q] * (k0 + c_hi * (k1 + k2 * c_hi));
      } else {
        a[q] = a[q] * ((k0 + kc * cl) - ks * sl);
        b[q] = b[q] * ((k0 + kc * ch) - ks * sh);
      }
    });
  }
  // decimation in frequency: a <- u, b <- v
  static_for<E>([&](auto q) {
    const cx<T> d = a[q] - b[q];
    a[q] = a[q] + b[q];
    b[q] = cmul(d, mul_w32<T, q>(wc0));
  });

  fft_passes<T, 12, false>(a, lds, twf, tid);  // a[q] = U[tid + 256q] = Z[2(tid + 256q)]
  __syncthreads();                            // the buffer is reused by the second transform
  fft_passes<T, 12, false>(b, lds, twf, tid);  // b[q] = V[tid + 256q] = Z[2(tid + 256q) + 1]

  // upper halves (k >= 2048) -> LDS: U[k] at k - 2048, V[k] at 2048 + (k - 2048)
  __syncthreads();
  static_for<E / 2>([&](auto q) {
    lds[tid + TP * q] = a[q + E / 2];
    lds[Q + tid + TP * q] = b[q + E / 2];
  });
  const cx<T> umid = a[E / 2];  // thread 0: U[2048] = Z[4096], the bin that pairs with itself
  __syncthreads();

  T *const arow = amp + (size_t)row * (size_t)(M + 1);
  const bool store_amp = !PEAK || amp != nullptr;
  // best: the forward bins, visited in ascending order; bestm: the mirrored bins, visited in descending order
  PeakBest<T> best{T(0), 0, cx<T>{T(0), T(0)}}, bestm{T(0), 0, cx<T>{T(0), T(0)}};
  T dc_amp = T(0);
  cx<T> dc_x{T(0), T(0)};
  typedef T V2 __attribute__((ext_vector_type(2)));
  // amplitude row as a buffer: pairs (2k, 2k+1) at byte 8 tid + 2048 q, mirrors (8191-2k, 8192-2k) at
  // byte 4 (M-1) - 8 tid - 2048 q = [4 (M-1) - 2048*7 - 8 tid] + 2048 (7 - q): two per-lane offsets, scalar rest
  typedef unsigned U2s __attribute__((ext_vector_type(2)));
  const __amdgpu_buffer_rsrc_t ws = __builtin_amdgcn_make_buffer_rsrc(arow, 0, (M + 1) * (int)sizeof(T), 0x00020000);
  const int vo_lo = tid * 8, vo_hi = 4 * (M - 1) - 2048 * 7 - tid * 8;
  static_for<E / 2>([&](auto qc) {
    constexpr int q = qc;
    const int k = tid + TP * q;  // < 2048
    // even bins: Z[2k] = U[k] with Z[8192 - 2k] = U[4096 - k] (k = 0: DC and Nyquist, paired with itself)
    const cx<T> ze = a[q];
    cx<T> zpe;
    if constexpr (q == 0) zpe = tid == 0 ? ze : lds[Q - tid];
    else zpe = lds[Q - TP * q - tid];
    // odd bins: Z[2k+1] = V[k] with Z[8191 - 2k] = V[4095 - k]
    const cx<T> zo = b[q];
    const cx<T> zpo = lds[Q + (Q - 1) - TP * q - tid];
    const cx<T> we = mul_w32<T, q>(wc0);  // W_16384^(2k)
    const cx<T> wo = mul_w32<T, q>(ws1);  // W_16384^(2k+1)
    // the frame came in pre-scaled by s_mid / 2: no multiplies here; DC and Nyquist (k = 0: not doubled) are fixed
    // up on their two values below
    const cx<T> ee = ze + conj(zpe), pe = cmul(ze - conj(zpe), we);
    const cx<T> eo = zo + conj(zpo), po = cmul(zo - conj(zpo), wo);
    cx<T> xae = add_mul_neg_i(ee, pe);        // scaled X[2k]
    cx<T> xbe = conj(add_mul_pos_i(ee, pe));  // scaled X[8192 - 2k]
    const cx<T> xao = add_mul_neg_i(eo, po);        // scaled X[2k + 1]
    const cx<T> xbo = conj(add_mul_pos_i(eo, po));  // scaled X[8191 - 2k]
    if constexpr (q == 0) {
      const T r = tid == 0 ? edge : T(1);  // k = 0 lives in thread 0's first pair
      xae = xae * r;
      xbe = xbe * r;
    }
    const T mae = mag(xae), mbe = mag(xbe), mao = mag(xao), mbo = mag(xbo);
    if constexpr (PEAK) {
      if (k == 0) {
        dc_amp = mae;
        dc_x = xae;
      } else {
        best.consider_ascending(mae, 2 * k, xae);
      }
      best.consider_ascending(mao, 2 * k + 1, xao);
      bestm.consider_descending(mbe, M - 2 * k, xbe);
      bestm.consider_descending(mbo, M - 1 - 2 * k, xbo);
    }
    if (store_amp) {
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(U2s, V2{mae, mao}), ws, vo_lo, 2048 * q, 2 /* nt */);
      __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(U2s, V2{mbo, mbe}), ws, vo_hi, 2048 * (7 - q), 2);
    }
  });
  // the middle bin 4096 = 2*2048 pairs with itself: X[4096] = conj(Z[4096]) = conj(U[2048])
  if (tid == 0) {
    const cx<T> xm = conj(umid);
    const T mm = mag(xm) * T(2);  // the pre-scaled frame carries s_mid / 2; this bin is one value, not a sum of two
    if constexpr (PEAK) best.consider(mm, H, xm);
    if (store_amp) arow[(unsigned)H] = mm;
  }

  if constexpr (PEAK) {
    best.consider(bestm.v, bestm.i, bestm.x);  // the thread's two runs, by the order-independent rule
    // Wave-wide arg-max in two scalar reductions instead of six rounds of the full rule on four shuffled values:
    // the largest value, then the smallest index among the lanes that hold it; that lane -- unique, a bin has one
    // owner -- hands its record to LDS itself, so the complex bin is never shuffled.  (Values are never NaN here: a
    // NaN never enters a PeakBest.)
    T vmax = best.v;
    static_for<6>([&](auto sc) { vmax = fmaxf(vmax, __shfl_xor(vmax, 32 >> sc, 64)); });
    const bool cand = vmax > T(0) && best.v == vmax;
    int imin = cand ? best.i : 0x7fffffff;
    static_for<6>([&](auto sc) { imin = min(imin, __shfl_xor(imin, 32 >> sc, 64)); });
    __shared__ T pk_v[4];
    __shared__ int pk_i[4];
    __shared__ cx<T> pk_x[4];
    const int wave = tid / 64;
    if (cand && best.i == imin) {
      pk_v[wave] = best.v;
      pk_i[wave] = best.i;
      pk_x[wave] = best.x;
    } else if ((tid & 63) == 0 && !(vmax > T(0))) {  // nothing > 0 in this wave's bins
      pk_v[wave] = T(0);
      pk_i[wave] = 0;
      pk_x[wave] = cx<T>{T(0), T(0)};
    }
    __syncthreads();
    if (tid == 0) {
      best = PeakBest<T>{pk_v[0], pk_i[0], pk_x[0]};
      static_for<3>([&](auto wc) { best.consider(pk_v[wc + 1], pk_i[wc + 1], pk_x[wc + 1]); });
      store_peak_fused(peaks, row, best, dc_amp, dc_x, freq_scale);
    }
  }
}

// The tail of the packed-real long-frame spectrum path: Z = the M-point transform (natural order, planar)
// of z[m] = x[2m] + i x[2m+1], M = N/2.  One lane takes the pair (k, M - k), 0 <= k <= M/2:
//   X[k]     =      (Z[k] + conj(Z[M-k])) / 2 - i W_N^k (Z[k] - conj(Z[M-k])) / 2
//   X[M - k] = conj((Z[k] + conj(Z[M-k])) / 2 + i W_N^k (Z[k] - conj(Z[M-k])) / 2),   Z[M] = Z[0]
// -- the same split spectrum_packed_kernel runs from LDS -- then magnitude + scaleAmplitude{One,Two}Sided
// (+ phase), spectrum.ts:45-72, :121-131; two-sided rows get X[N - k] = conj(X[k]) as well.
//   W_N^k = twa[k >> 9] * twb[k & 511] (the N-point plan's two-level table); bins = M + 1 or N.
// One lane takes k = 4i .. 4i+3 (M/8 lanes per frame, M >= 2048): 16-byte loads of Z[4i ..] and of
// Z[M-4i-4 .. M-4i-1] (the mirrors of 4i+1 .. 4i+3; Z[M-4i] is one more dword, Z[0] for lane 0), 16-byte
// stores of bins 4i .. 4i+3 and M-4i-3 .. M-4i (rows of M + 1 bins: 4-byte aligned); lane 0 adds bin M/2.
template <typename T>
__global__ void __launch_bounds__(256)
split_amp_rows_kernel(const T *__restrict__ zre, const T *__restrict__ zim, T *__restrict__ amp, T *__restrict__ ph,
                      const cx<T> *__restrict__ twa, const cx<T> *__restrict__ twb, const int M, const int bins,
                      const T s_edge, const T s_mid, const long long batch) {
  typedef T V4 __attribute__((ext_vector_type(4)));
  typedef T V4u __attribute__((ext_vector_type(4), aligned(4)));  // rows of M + 1 bins start anywhere
  const int chunks = M / 8 / 256;
  const long long b = (long long)blockIdx.x / chunks;
  const int i = (int)((long long)blockIdx.x % chunks) * 256 + (int)threadIdx.x;
  if (b >= batch) return;
  const T *const re = zre + (size_t)b * (size_t)M, *const im = zim + (size_t)b * (size_t)M;
  T *const arow = amp + (size_t)b * (size_t)bins;
  T *const prow = ph ? ph + (size_t)b * (size_t)bins : nullptr;
  const bool two = bins > M + 1;
  const int k0 = 4 * i;
  const V4 fr = ld_stream(reinterpret_cast<const V4 *>(re + k0)), fi = ld_stream(reinterpret_cast<const V4 *>(im + k0));
  const V4 mr = ld_stream(reinterpret_cast<const V4 *>(re + (M - k0 - 4)));
  const V4 mi = ld_stream(reinterpret_cast<const V4 *>(im + (M - k0 - 4)));
  const int km = (M - k0) & (M - 1);
  const cx<T> m0{ld_stream(re + km), ld_stream(im + km)};
  const cx<T> zh{re[M / 2], im[M / 2]};  // lane 0's extra bin (every lane loads it: no branch around a load)
  const cx<T> wa = twa[k0 >> 9];
  const V4 wb01 = *reinterpret_cast<const V4 *>(twb + (k0 & 511)), wb23 = *(reinterpret_cast<const V4 *>(twb + (k0 & 511)) + 1);
  const cx<T> z[4] = {cx<T>{fr.x, fi.x}, cx<T>{fr.y, fi.y}, cx<T>{fr.z, fi.z}, cx<T>{fr.w, fi.w}};
  const cx<T> zp[4] = {m0, cx<T>{mr.w, mi.w}, cx<T>{mr.z, mi.z}, cx<T>{mr.y, mi.y}};
  const cx<T> wb[4] = {cx<T>{wb01.x, wb01.y}, cx<T>{wb01.z, wb01.w}, cx<T>{wb23.x, wb23.y}, cx<T>{wb23.z, wb23.w}};
  cx<T> xa[4], xb[4];
  T ma[4], mb[4];
  static_for<4>([&](auto j) {
    const cx<T> w = cmul(wa, wb[j]);
    const cx<T> e = (z[j] + conj(zp[j])) * T(0.5), p = cmul(z[j] - conj(zp[j]), w) * T(0.5);
    xa[j] = add_mul_neg_i(e, p), xb[j] = conj(add_mul_pos_i(e, p));  // X[k], X[M - k]
    const T sc = (j == 0 && i == 0) ? s_edge : s_mid;                // k = 0 <-> bins 0 and M: DC and Nyquist
    ma[j] = mag(xa[j]) * sc, mb[j] = mag(xb[j]) * sc;
  });
  *reinterpret_cast<V4u *>(arow + k0) = V4{ma[0], ma[1], ma[2], ma[3]};
  *reinterpret_cast<V4u *>(arow + (M - k0 - 3)) = V4{mb[3], mb[2], mb[1], mb[0]};
  if (prow) {
    *reinterpret_cast<V4u *>(prow + k0) =
        V4{T(atan2(xa[0].y, xa[0].x)), T(atan2(xa[1].y, xa[1].x)), T(atan2(xa[2].y, xa[2].x)), T(atan2(xa[3].y, xa[3].x))};
    *reinterpret_cast<V4u *>(prow + (M - k0 - 3)) =
        V4{T(atan2(xb[3].y, xb[3].x)), T(atan2(xb[2].y, xb[2].x)), T(atan2(xb[1].y, xb[1].x)), T(atan2(xb[0].y, xb[0].x))};
  }
  if (two) {  // X[N - k] = conj(X[k]) (k > 0), X[M + k] = conj(X[M - k])
    static_for<4>([&](auto j) {
      const int k = k0 + j;
      if (k > 0) {
        arow[2 * M - k] = ma[j];
        arow[M + k] = mb[j];
        if (prow) {
          prow[2 * M - k] = T(atan2(-xa[j].y, xa[j].x));
          prow[M + k] = T(atan2(-xb[j].y, xb[j].x));
        }
      }
    });
  }
  if (i == 0) {  // X[M/2] = conj(Z[M/2]) pairs with itself
    arow[M / 2] = mag(zh) * s_mid;
    if (prow) prow[M / 2] = T(atan2(-zh.y, zh.x));
    if (two) {
      arow[M + M / 2] = mag(zh) * s_mid;
      if (prow) prow[M + M / 2] = T(atan2(zh.y, zh.x));
    }
  }
}

}  // namespace pdsp

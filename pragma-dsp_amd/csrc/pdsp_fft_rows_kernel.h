// pdsp_fft_rows_kernel.h -- rows in one pass over HBM: the Stockham kernel, its staged, split, paired and packed-real forms.
#pragma once

#include "pdsp_fft_core.h"
#include "pdsp_packed.h"

namespace pdsp {

// ---- load / store policies ------------------------------------------------

// ld(row, off, lane) -> cx: fetch point off + lane of row `row` (row < batch).
// st(row, off, lane, cx): write point off + lane.
// `row` and `off` are wave-uniform whenever a transform spans whole waves, so
// `base + row*N + off` stays in SGPRs and the only per-lane address register is
// `lane` (global_load ... v_lane, s[base:base+1] offset:imm).

template <typename T>
struct LoadComplex {  // forwardComplex / inverse (planes swapped by the caller)
  const T *__restrict__ re;
  const T *__restrict__ im;
  long long n;
  __device__ __forceinline__ cx<T> operator()(long long row, int off, int lane) const {
    const size_t o = (size_t)row * (size_t)n + (size_t)off;
    return cx<T>{ld_stream(re + o + (unsigned)lane), ld_stream(im + o + (unsigned)lane)};
  }
  static constexpr bool kPlanar = true;  // rows are contiguous planes: eligible for staged I/O
  static constexpr bool kHasIm = true;
  static constexpr bool kPacked = false;
  __device__ __forceinline__ const T *plane_re() const { return re; }
  __device__ __forceinline__ const T *plane_im() const { return im; }
};

template <typename T>
struct LoadReal {  // Radix2Fft.forward: imaginary part is zero
  const T *__restrict__ re;
  long long n;
  __device__ __forceinline__ cx<T> operator()(long long row, int off, int lane) const {
    return cx<T>{ld_stream(re + (size_t)row * (size_t)n + (size_t)off + (unsigned)lane), T(0)};
  }
  static constexpr bool kPlanar = true;
  static constexpr bool kHasIm = false;
  static constexpr bool kPacked = false;
  __device__ __forceinline__ const T *plane_re() const { return re; }
  __device__ __forceinline__ const T *plane_im() const { return nullptr; }
};

// Interleaved (re, im) rows -- the layout of I/Q streams and of complex64 tensors; one 8-byte
// access per point.  CONJ turns the forward kernel into the inverse: conj on the way in and out.
template <typename T, bool CONJ>
struct LoadInterleaved {
  const cx<T> *__restrict__ z;
  long long n;
  __device__ __forceinline__ cx<T> operator()(long long row, int off, int lane) const {
    cx<T> v = ld_stream(z + (size_t)row * (size_t)n + (size_t)off + (unsigned)lane);
    if constexpr (CONJ) v.y = -v.y;
    return v;
  }
  static constexpr bool kPlanar = false;
  static constexpr bool kHasIm = true;
};

template <typename T, bool CONJ>
struct StoreInterleaved {
  cx<T> *__restrict__ z;
  long long n;
  T scale;
  __device__ __forceinline__ void operator()(long long row, int off, int lane, cx<T> v) const {
    v = v * scale;
    if constexpr (CONJ) v.y = -v.y;
    st_stream(v, z + (size_t)row * (size_t)n + (size_t)off + (unsigned)lane);
  }
  static constexpr bool kPlanar = false;
};

template <typename T>
struct StoreComplex {
  T *__restrict__ re;
  T *__restrict__ im;
  long long n;
  T scale;  // 1 forward, 1/N inverse (fft.ts:142-148); power of two => exact
  __device__ __forceinline__ void operator()(long long row, int off, int lane, cx<T> v) const {
    const size_t o = (size_t)row * (size_t)n + (size_t)off;
    v = v * scale;
    st_stream(v.x, re + o + (unsigned)lane);
    st_stream(v.y, im + o + (unsigned)lane);
  }
  static constexpr bool kPlanar = true;
};

// ---- the kernels ---------------------------------------------------------------

template <typename T, int LOG2N, class LD, class ST>
__global__ void __launch_bounds__(FftTraits<LOG2N>::WG)
fft_stockham_kernel(const LD ld, const ST st, const typename vec2<T>::type *__restrict__ tw,
                    const long long batch) {
  using TR = FftTraits<LOG2N>;
  constexpr int E = TR::E, TP = TR::TP, NP = TR::NP;

  __shared__ cx<T> lds[TR::LDS_ELEMS];

  const int tid = TP == 1 ? 0 : (int)(threadIdx.x % TP);
  const int rloc = (int)(threadIdx.x / TP);
  const long long row_raw = (long long)blockIdx.x * TR::ROWS + rloc;
  const bool live = row_raw < batch;
  // dead rows of the last workgroup recompute the last live row and skip the
  // store, so that every thread reaches every barrier without predicated loads
  const long long row = uniform_row<TP>(live ? row_raw : batch - 1);
  cx<T> *const lrow = lds + (NP > 1 ? rloc * TR::LROW : 0);

  cx<T> x[E];
  constexpr bool kRegTw = (TP >= 16 && NP > 1);  // twiddle bases in registers, fetched with the row loads
  std::conditional_t<kRegTw, RegTwiddles<T, LOG2N>, TableTwiddles<T, LOG2N>> twf;
  static_for<E>([&](auto q) { x[q] = ld(row, TP * q, tid); });
  if constexpr (kRegTw) twf.load(reinterpret_cast<const cx<T> *>(tw), tid);  // behind the row loads
  if constexpr (!kRegTw) twf.tw = reinterpret_cast<const cx<T> *>(tw);
  fft_passes<T, LOG2N, false>(x, lrow, twf, tid);
  if (live) {
    static_for<E>([&](auto q) { st(row, TP * q, tid, x[q]); });
  }
}

// Small transforms (32 <= N <= 256): only N/16 <= 16 threads own a row, so the direct kernel's
// wave-level loads are 16..64-byte fragments of many rows (N = 64 measured 15 % of the HBM
// roofline).  But the 4096/N rows of a workgroup are ONE contiguous 4096-point chunk per plane:
// stage it through LDS with perfectly coalesced 16-byte accesses on both sides -- one extra LDS
// round trip each way, cheap next to the few passes such a size needs.
//   LD/ST must be the planar policies (kPlanar) over 16-byte aligned planes.
template <typename T, int LOG2N, class LD, class ST>
__global__ void __launch_bounds__(256)
fft_staged_kernel(const LD ld, const ST st, const typename vec2<T>::type *__restrict__ tw, const long long batch) {
  using TR = FftTraits<LOG2N>;
  constexpr int N = TR::N, E = TR::E, TP = TR::TP, ROWS = TR::ROWS, WG = 256;
  static_assert(TR::WG == WG && TR::NP > 1 && N % 16 == 0, "staged path: 32 <= N <= 256");
  constexpr int CHUNK = ROWS * N;  // 4096 points per plane
  typedef T V4 __attribute__((ext_vector_type(4)));
  __shared__ cx<T> lds[TR::LDS_ELEMS];

  const int t = (int)threadIdx.x;
  const int tid = t % TP, rloc = t / TP;
  cx<T> *const lrow = lds + rloc * TR::LROW;
  const size_t base = (size_t)blockIdx.x * CHUNK;
  const size_t limit = (size_t)batch * N;  // points per plane; a multiple of 4
  const T *const pre = ld.plane_re();
  const T *const pim = ld.plane_im();

  // chunk -> LDS in natural order: point p of the chunk is element p % N of local row p / N
  static_for<CHUNK / 4 / WG>([&](auto ic) {
    const int p = 4 * (t + WG * ic);
    size_t g = base + (size_t)p;
    g = g + 4 <= limit ? g : limit - 4;  // the tail workgroup re-reads valid points; its dead rows never store
    const V4 r = ld_stream(reinterpret_cast<const V4 *>(pre + g));
    V4 m = V4{T(0), T(0), T(0), T(0)};
    if constexpr (LD::kHasIm) m = ld_stream(reinterpret_cast<const V4 *>(pim + g));  // no run-time branch around a load
    cx<T> *const d = lds + (p / N) * TR::LROW + lds_pad(p % N);  // 4 points never straddle a 16-block
    d[0] = cx<T>{r.x, m.x};
    d[1] = cx<T>{r.y, m.y};
    d[2] = cx<T>{r.z, m.z};
    d[3] = cx<T>{r.w, m.w};
  });
  __syncthreads();
  cx<T> x[E];
  {
    const cx<T> *const rbase = lrow + lds_pad(tid);
    static_for<E>([&](auto q) { x[q] = rbase[cpad(TP * q)]; });
  }
  __syncthreads();  // the first pass scatters into the same buffer

  RegTwiddles<T, LOG2N> twf;
  twf.load(reinterpret_cast<const cx<T> *>(tw), tid);
  fft_passes<T, LOG2N, true>(x, lrow, twf, tid);  // result in LDS, natural order per row
  __syncthreads();

  static_for<CHUNK / 4 / WG>([&](auto ic) {
    const int p = 4 * (t + WG * ic);
    const size_t g = base + (size_t)p;
    if (g + 4 <= limit) {
      const cx<T> *const d = lds + (p / N) * TR::LROW + lds_pad(p % N);
      const cx<T> v0 = d[0] * st.scale, v1 = d[1] * st.scale, v2 = d[2] * st.scale, v3 = d[3] * st.scale;
      st_stream(V4{v0.x, v1.x, v2.x, v3.x}, reinterpret_cast<V4 *>(st.re + g));
      st_stream(V4{v0.y, v1.y, v2.y, v3.y}, reinterpret_cast<V4 *>(st.im + g));
    }
  });
}

// Tiny transforms (2 <= N <= 16; the amplitude spectrum also N = 32): one thread owns a whole row, so in the direct kernel a lane's
// accesses are N*4 bytes apart (N = 16 measured 4 % of the HBM roofline).  Same cure as
// fft_staged_kernel: the workgroup's 4096-point chunk goes through LDS with coalesced 16-byte
// accesses on both sides; each thread transforms 16/N rows out of LDS in registers (fft_reg).
//   AMP = false: planar complex rows out (times st.scale) -- forward / forwardComplex / inverse.
//   AMP = true:  real frames (whole, contiguous) times an optional window in, one- or two-sided
//                amplitude rows of `bins` values out (the body of spectrum(), complex kernel on (x*w, 0)).
template <typename T, int LOG2N, bool AMP, class LD>
__global__ void __launch_bounds__(256)
fft_tiny_staged_kernel(const LD ld, const T *__restrict__ win, T *__restrict__ o1, T *__restrict__ o2, const T scale,
                       const int bins, const int nyq, const T s_edge, const T s_mid, const long long batch) {
  constexpr int N = 1 << LOG2N, WG = 256, CHUNK = 4096, ROWS = CHUNK / N, RPT = ROWS >= WG ? ROWS / WG : 1;
  static_assert(LOG2N >= 1 && LOG2N <= 5, "tiny path: 2 <= N <= 32 (N = 32: half the threads hold a row)");
  typedef T V4 __attribute__((ext_vector_type(4)));
  __shared__ cx<T> lds[CHUNK + CHUNK / 16];
  const int t = (int)threadIdx.x;
  const size_t base = (size_t)blockIdx.x * CHUNK;
  const size_t limit = (size_t)batch * N;  // points per plane
  const T *const pre = ld.plane_re();
  const T *const pim = ld.plane_im();

  static_for<CHUNK / 4 / WG>([&](auto ic) {
    const int p = 4 * (t + WG * ic);
    size_t g = base + (size_t)p;
    if (limit >= 4) g = g + 4 <= limit ? g : limit - 4;  // the tail workgroup re-reads valid points
    V4 r, m = V4{T(0), T(0), T(0), T(0)};
    if (limit >= 4) {
      r = ld_stream(reinterpret_cast<const V4 *>(pre + g));
      if constexpr (LD::kHasIm) m = ld_stream(reinterpret_cast<const V4 *>(pim + g));
    } else {  // a single N = 2 row: two points in all
      r = V4{pre[0], pre[1], T(0), T(0)};
      if constexpr (LD::kHasIm) m = V4{pim[0], pim[1], T(0), T(0)};
    }
    if constexpr (N == 2) {
      // an odd number of 2-point rows: the group that straddles the end was read two points early
      const size_t g0 = base + (size_t)p;
      if (limit >= 4 && g0 < limit && g0 + 4 > limit) {
        r = V4{r.z, r.w, T(0), T(0)};
        m = V4{m.z, m.w, T(0), T(0)};
      }
    }
    cx<T> *const d = lds + lds_pad(p);
    d[0] = cx<T>{r.x, m.x};
    d[1] = cx<T>{r.y, m.y};
    d[2] = cx<T>{r.z, m.z};
    d[3] = cx<T>{r.w, m.w};
  });
  __syncthreads();

  cx<T> x[RPT][N];
  const bool holds_row = ROWS >= WG || t < ROWS;
  static_for<RPT>([&](auto rc) {
    const int row = holds_row ? t + WG * rc : ROWS - 1;  // local row; its points are lds[pad(row*N + q)]
    static_for<N>([&](auto q) {
      cx<T> v = lds[lds_pad(row * N + q)];
      if constexpr (AMP) {
        if (win) v = v * win[q];  // uniform across the lanes: scalar loads
      }
      x[rc][q] = v;
    });
    fft_reg<T, N>(x[rc]);  // X[k] in slot bitrev(k)
  });
  __syncthreads();  // every thread has its inputs: the buffer now takes the outputs

  if constexpr (!AMP) {
    static_for<RPT>([&](auto rc) {
      const int row = t + WG * rc;
      if (holds_row) static_for<N>([&](auto k) { lds[lds_pad(row * N + k)] = x[rc][bitrev(k, LOG2N)] * scale; });
    });
    __syncthreads();
    static_for<CHUNK / 4 / WG>([&](auto ic) {
      const int p = 4 * (t + WG * ic);
      const size_t g = base + (size_t)p;
      const cx<T> *const d = lds + lds_pad(p);
      if (g + 4 <= limit) {
        st_stream(V4{d[0].x, d[1].x, d[2].x, d[3].x}, reinterpret_cast<V4 *>(o1 + g));
        st_stream(V4{d[0].y, d[1].y, d[2].y, d[3].y}, reinterpret_cast<V4 *>(o2 + g));
      } else if (g < limit) {  // N = 2, odd tail: fewer than four points left
        for (int j = 0; j < 4 && g + j < limit; ++j) {
          o1[g + j] = d[j].x;
          o2[g + j] = d[j].y;
        }
      }
    });
  } else {
    T *const ampf = reinterpret_cast<T *>(lds);  // ROWS rows of `bins` <= N amplitudes: at most 4096 values
    static_for<RPT>([&](auto rc) {
      const int row = t + WG * rc;
      static_for<N>([&](auto k) {
        if (holds_row && k < bins)
          ampf[row * bins + k] = mag(x[rc][bitrev(k, LOG2N)]) * ((k == 0 || k == nyq) ? s_edge : s_mid);
      });
    });
    __syncthreads();
    const size_t out_base = (size_t)blockIdx.x * ROWS * (size_t)bins, out_limit = (size_t)batch * (size_t)bins;
    const int out_count = ROWS * bins;
    for (int i = t; i < out_count; i += WG)
      if (out_base + (size_t)i < out_limit) o1[out_base + (size_t)i] = ampf[i];
  }
}

// Radix2Fft.forward(real input) (src/core/fft.ts:77-79: imaginary part taken as zero) on rows of N = 2M real
// samples through the packed-real identity, with the FULL complex spectrum written to both planes.
//   z[m] = x[2m] + i x[2m+1] (an 8-byte view of the row),  Z = FFT_M(z)  -- half the butterflies, LDS traffic and
//   twiddles of running the complex kernel on (x, 0), and the row arrives as 8-byte instead of 4-byte loads;
//   E[k] = (Z[k] + conj Z[M-k]) / 2,  O[k] = (Z[k] - conj Z[M-k]) / (2i)   (transforms of the even / odd samples)
//   X[k] = E[k] + W_N^k O[k],  X[k + M] = E[k] - W_N^k O[k],   0 <= k < M.
// Every thread forms X[k], X[k + M] for its OWN sixteen k = tid + TP q from (Z[k], Z[M-k]) read back from LDS: each
// pair (k, M-k) is split twice, once from either side -- six packed instructions per k -- so that both planes
// leave as the same forward unit-stride streams `row N + tid + TP q` the complex kernel writes.  (Round 2 tried the
// split that writes X[k] and its mirror X[N-k] = conj X[k] from one side: four store streams per plane in two
// directions, slower than the complex kernel at every size)
//   tw = radix table of the M-point transform (Tables::tw_half), twr[k] = W_N^k (Tables::twr), scale = 1.
// Rows must be aligned to one pair of samples.  In place row for row is fine: a workgroup loads its rows before it
// stores.  Dispatched for f64 rows (the drop-in's default arithmetic) of N = 8192 and N = 16384, the sizes where the
// complex kernel is short of registers or LDS (N = 8192: 50-62 -> 71-82 % of 8 TB/s by box; N = 16384: one pass
// instead of a four-step transform, 20 -> 63-65 %).  Below 8192 it measured +-: +1 ... +9 % on one box, -9 ... +2 %
// on another; in f32 both forms run at the box's copy ceiling (A/B 0.98 ... 1.01): neither is built.
template <typename T, int LOG2M>
__global__ void __launch_bounds__(kPackedWG<LOG2M>)
fft_real_kernel(const T *__restrict__ xin, T *__restrict__ ore, T *__restrict__ oim, const T scale,
                const typename vec2<T>::type *__restrict__ tw, const typename vec2<T>::type *__restrict__ twr,
                const long long batch) {
  using PR = PackedRow<T, LOG2M>;
  constexpr int E = PR::E, TP = PR::TP, M = PR::M;
  static_assert(LOG2M >= 8 && TP % 16 == 0, "N >= 512: register twiddle bases, constant LDS offsets");
  __shared__ cx<T> lds[PR::TR::LDS_ELEMS];

  const PR pr(lds, batch);
  const int tid = pr.tid;
  PackedTwiddles<T, LOG2M> twd;
  const cx<T> *const x2 = reinterpret_cast<const cx<T> *>(xin + (size_t)pr.row * (size_t)(2 * M));
  cx<T> x[E];
  static_for<E>([&](auto q) { x[q] = ld_stream(x2 + TP * q + (unsigned)tid); });
  twd.load(tw, twr, tid);  // the tables behind the row loads (load_order_fence's header)

  fft_passes<T, LOG2M, true, PR::LOG2E>(x, pr.lrow, twd.twf, tid);  // Z in LDS, natural order
  __syncthreads();

  T *const rre = ore + (size_t)pr.row * (size_t)(2 * M), *const rim = oim + (size_t)pr.row * (size_t)(2 * M);
  const T h = T(0.5) * scale;
  const auto pairs = pr.pairs(pr.lrow);
  static_for<E>([&](auto qc) {
    constexpr int q = qc;
    const auto sp = pairs.forward_split(qc, tid + TP * q, (M - tid - TP * q) & (M - 1));
    const cx<T> w = twd.wk(qc);
    const cx<T> s = sp.s(), p = sp.p(w);               // S, 2i W^k O[k]
    const cx<T> xa = add_mul_neg_i(s, p) * h;          // X[k]     = (S - i P) / 2
    const cx<T> xb = add_mul_pos_i(s, p) * h;          // X[k + M] = (S + i P) / 2
    if (pr.live) {
      st_stream(xa.x, rre + TP * q + (unsigned)tid);
      st_stream(xa.y, rim + TP * q + (unsigned)tid);
      st_stream(xb.x, rre + M + TP * q + (unsigned)tid);
      st_stream(xb.y, rim + M + TP * q + (unsigned)tid);
    }
  });
}

// forward / forwardComplex / inverse at N = 16384 (f32), re-cut so that TWO workgroups fit a CU.
// fft_stockham_kernel<14> needs 139 KB of LDS: one 1024-thread workgroup per CU whose load, compute
// and store phases cannot overlap anything (52 % of the HBM roofline, against 77 % at N = 4096).
// Here the transform is one radix-4 decimation-in-time step over four 4096-point transforms that
// the SAME 256 threads run back to back through one 4096-point LDS buffer:
//   one 16-byte load per plane gives x[4m..4m+3] = (s0[m], s1[m], s2[m], s3[m]);  Fj = FFT_4096(sj);
//   X[k + 4096q] = sum_j (-i)^{jq} W_16384^{jk} Fj[k]   in registers (thread tid holds k = tid + 256e
//   of all four).
// 34.8 KB of LDS and ~200 VGPRs per thread: two workgroups per CU, 16-byte loads, and one
// workgroup's HBM phases overlap the other's butterflies.
//   tw12 = radix table of the 4096-point transform; tws[k] = W_16384^k, k < 768.
template <typename T, int LOG2S, class LD, class ST>
__global__ void __launch_bounds__((1 << LOG2S) / 16, 2)
fft_split4_kernel(const LD ld, const ST st, const typename vec2<T>::type *__restrict__ tw12,
                  const typename vec2<T>::type *__restrict__ tws, const long long batch) {
  using TR = FftTraits<LOG2S>;
  constexpr int E = 16, TP = TR::TP, H = TR::N, N = 4 * H;
  static_assert(LD::kPlanar && ST::kPlanar, "planar rows");
  static_assert(TP >= 64 && TP % 64 == 0, "whole waves per row");
  typedef T V4 __attribute__((ext_vector_type(4)));
  __shared__ cx<T> lds[TR::LROW];

  const int tid = (int)threadIdx.x;
  const long long row = uniform_row<TP>((long long)blockIdx.x);
  if (row >= batch) return;

  cx<T> a[E], b[E], c[E], d[E];
  RegTwiddles<T, LOG2S> twf;
  const cx<T> *const twn = reinterpret_cast<const cx<T> *>(tws);
  cx<T> w1, w2, w3;
  twf.load(reinterpret_cast<const cx<T> *>(tw12), tid);  // tables first (load_order_fence's header)
  w1 = twn[(unsigned)tid], w2 = twn[(unsigned)(2 * tid)], w3 = twn[(unsigned)(3 * tid)];
  load_order_fence();
  if constexpr (LD::kPacked) {
    // points 4m .. 4m+3 = samples 8m .. 8m+7 of the frame: two 16-byte loads (+ two of the window table)
    const V4 *const f4 = reinterpret_cast<const V4 *>(ld.x + (size_t)row * (size_t)ld.stride);
    cx<T> wcs{T(1), T(0)};
    if constexpr (LD::kWin >= 2) wcs = reinterpret_cast<const cx<T> *>(ld.wb)[(unsigned)tid];
    static_for<E>([&](auto q) {
      // plain loads: the two halves of a lane's 32 bytes come from one cache line in two instructions, and
      // the second finds it in L1 (non-temporal: -8 %, tools/ab_long_spectrum.py at N = 32768)
      V4 r0 = f4[2 * (TP * q + (unsigned)tid)], r1 = f4[2 * (TP * q + (unsigned)tid) + 1];
      if constexpr (LD::kWin == 1) {
        const V4 *const w4 = reinterpret_cast<const V4 *>(ld.win);
        r0 = r0 * w4[2 * (TP * q + (unsigned)tid)];
        r1 = r1 * w4[2 * (TP * q + (unsigned)tid) + 1];
      }
      if constexpr (LD::kWin >= 2) {
        static_assert(LD::kWin < 2 || (sizeof(T) == 4 && TP == 256), "fused windows: f32 rows of 16384 points");
        const cx<T> c0 = cmul(wcs, reinterpret_cast<const cx<T> *>(ld.wq)[q]);  // wave-uniform: scalar loads
        cx<T> w[4];
        fused_window_pairs<T, LD::kWin == 3>(c0, reinterpret_cast<const cx<T> *>(ld.we), ld.k0, ld.k1, ld.k2, w);
        r0 = r0 * V4{w[0].x, w[0].y, w[1].x, w[1].y};
        r1 = r1 * V4{w[2].x, w[2].y, w[3].x, w[3].y};
      }
      a[q] = cx<T>{r0.x, r0.y};
      b[q] = cx<T>{r0.z, r0.w};
      c[q] = cx<T>{r1.x, r1.y};
      d[q] = cx<T>{r1.z, r1.w};
      // window table: a step holds four 16-byte loads; left alone hipcc hoists all sixteen steps' loads above the
      // first product (256 registers in flight beside the 128 of a..d: 10 spilled).  Four steps at a time.
      if constexpr (LD::kWin == 1 && q % 4 == 3) load_order_fence();
    });
  } else if constexpr (LD::kHasIm) {
    const V4 *const r4 = reinterpret_cast<const V4 *>(ld.plane_re() + (size_t)row * N);
    const V4 *const i4 = reinterpret_cast<const V4 *>(ld.plane_im() + (size_t)row * N);
    static_for<E>([&](auto q) {
      const V4 r = ld_stream(r4 + TP * q + (unsigned)tid);
      const V4 m = ld_stream(i4 + TP * q + (unsigned)tid);
      a[q] = cx<T>{r.x, m.x};
      b[q] = cx<T>{r.y, m.y};
      c[q] = cx<T>{r.z, m.z};
      d[q] = cx<T>{r.w, m.w};
    });
  } else {
    const V4 *const r4 = reinterpret_cast<const V4 *>(ld.plane_re() + (size_t)row * N);
    static_for<E>([&](auto q) {
      const V4 r = ld_stream(r4 + TP * q + (unsigned)tid);
      a[q] = cx<T>{r.x, T(0)};
      b[q] = cx<T>{r.y, T(0)};
      c[q] = cx<T>{r.z, T(0)};
      d[q] = cx<T>{r.w, T(0)};
    });
  }

  fft_passes<T, LOG2S, false>(a, lds, twf, tid);  // a[e] = F0[tid + TP*e]
  __syncthreads();                               // the buffer is reused by the next transform
  fft_passes<T, LOG2S, false>(b, lds, twf, tid);
  __syncthreads();
  fft_passes<T, LOG2S, false>(c, lds, twf, tid);
  __syncthreads();
  fft_passes<T, LOG2S, false>(d, lds, twf, tid);

  // radix-4 combine; W_N^{j(tid + TP*e)} = wj * W_64^{je}  (N = 64*TP)
  static_for<E>([&](auto ec) {
    constexpr int e = ec;
    const cx<T> t1 = cmul(b[e], mul_w64<T, e>(w1));
    const cx<T> t2 = cmul(c[e], mul_w64<T, (2 * e) % 64>(w2));
    const cx<T> t3 = cmul(d[e], mul_w64<T, (3 * e) % 64>(w3));
    const cx<T> s0 = a[e] + t2, s1 = a[e] - t2, s2 = t1 + t3, d13 = t1 - t3;
    st(row, 0 * H + TP * e, tid, s0 + s2);
    st(row, 1 * H + TP * e, tid, add_mul_neg_i(s1, d13));  // s1 - i (t1 - t3)
    st(row, 2 * H + TP * e, tid, s0 - s2);
    st(row, 3 * H + TP * e, tid, add_mul_pos_i(s1, d13));  // s1 + i (t1 - t3)
  });
}

// N = P * 16384 (P = 2, 4) in ONE pass over HBM, by workgroups that are siblings in one XCD's L2.
// Decimation in frequency by P in front of fft_split4_kernel's body: with S = 16384 and n < S,
//   y_h[n] = W_N^(h n) * sum_{p < P} x[n + p S] W_P^(p h),        X[P k + h] = FFT_S(y_h)[k],     h < P,
// so transform t is P independent 16384-point transforms -- P workgroups -- each of which reads ALL of x (P
// contiguous segments of S points) and writes every P-th output.  Taken alone that is P times the read traffic
// and partial-line writes; but an XCD's workgroups share its 4 MiB L2, and the dispatcher deals workgroup ids
// round-robin to the eight XCDs: sibling h of transform t sits at blockIdx (t / 8) * 8 P + 8 h + (t % 8), so the
// P siblings have the same id mod 8 -- the same XCD -- and leave the dispatcher one round apart.  They run the
// same instruction stream over the same addresses: the first sibling's loads bring a line into that L2, the others
// hit it; each line of the output is completed there by the P siblings' stores before it is written back.  HBM
// then sees 8 B read + 8 B written per sample -- one pass -- where the tile passes make two (32 B).
// (If the dispatcher did not pair them the results would still be right: every workgroup is self-sufficient.)
//   tw12 = radix table of the 4096-point transform; tws[k] = W_16384^k, k < 768 (fft_split4_kernel's);
//   W_N^m = twa[m >> 9] * twb[m & 511]; REAL: Radix2Fft.forward rows (no imaginary plane).
// PK > 0: the rows are PACKED real frames (LoadPackedFrames' layout: point m = (x[2m], x[2m+1]) of a frame of 2N
// samples, `pk.stride` samples apart) -- the one transform pass of spectrum() on frames of 2 * P * 16384 samples,
// split_amp_rows_kernel undoes the packing -- times the window: PK - 1 = 0 rect, 1 window table (in_im), 2 / 3
// two- / three-term cosine-sum window evaluated in registers (LoadPackedFrames' tables; segment p adds the angle
// 32768 f p = 2 * (8 * 2048 f)).  twa / twb then belong to the plan of 2N points: W_N^m = W_2N^(2m).
struct PairedPacked {
  long long stride;
  const float *wb, *wq, *we;
  float k0, k1, k2;
};
template <typename T, int LOG2P, bool REAL, int PK = 0>
__global__ void __launch_bounds__(256, 2)
fft_paired_kernel(const T *__restrict__ in_re, const T *__restrict__ in_im, T *__restrict__ out_re, T *__restrict__ out_im,
                  const typename vec2<T>::type *__restrict__ tw12, const typename vec2<T>::type *__restrict__ tws,
                  const cx<T> *__restrict__ twa, const cx<T> *__restrict__ twb, const T scale, const long long batch,
                  const PairedPacked pk) {
  static_assert(PK == 0 || (!REAL && sizeof(T) == 4 && LOG2P == 1), "packed frames: f32, two siblings");
  constexpr unsigned TSH = PK ? 1u : 0u;
  using TR = FftTraits<12>;
  constexpr int E = 16, TP = 256, H = 4096, S = 4 * H, P = 1 << LOG2P, N = P * S;
  static_assert(LOG2P == 1 || LOG2P == 2, "two or four siblings");
  typedef T V4 __attribute__((ext_vector_type(4)));
  __shared__ cx<T> lds[TR::LROW];

  const int tid = (int)threadIdx.x;
  const unsigned blk = (unsigned)__builtin_amdgcn_readfirstlane((int)blockIdx.x);
  const long long t = (long long)(blk / (8u * P)) * 8 + (blk & 7u);
  const unsigned h = (blk >> 3) & (unsigned)(P - 1);
  if (t >= batch) return;

  RegTwiddles<T, 12> twf;
  twf.load(reinterpret_cast<const cx<T> *>(tw12), tid);
  const cx<T> *const twn = reinterpret_cast<const cx<T> *>(tws);
  const cx<T> w1 = twn[(unsigned)tid], w2 = twn[(unsigned)(2 * tid)], w3 = twn[(unsigned)(3 * tid)];
  // W_N^(h n), n = 4 (tid + 256 q) + j:  wt[j] = W_N^(h (4 tid + j)) per thread, wq = W_N^(1024 h q) per q (wave-uniform)
  auto look = [&](unsigned m) { return cmul(twa[(m << TSH) >> 9], twb[(m << TSH) & 511]); };
  cx<T> wt[4];
  static_for<4>([&](auto j) { wt[j] = look(h * (unsigned)(4 * tid + j)); });
  cx<T> wcs{T(1), T(0)}, wseg{T(1), T(0)};  // PK >= 3: cs(8 f tid); cs(32768 f) = cs(8 * 2048 f)^2
  if constexpr (PK >= 3) {
    wcs = reinterpret_cast<const cx<T> *>(pk.wb)[(unsigned)tid];
    const cx<T> w8 = reinterpret_cast<const cx<T> *>(pk.wq)[8];
    wseg = cmul(w8, w8);
  }
  load_order_fence();

  const size_t base = (size_t)t * (size_t)N;
  cx<T> a[E], b[E], c[E], d[E];
  // The loads run AHEAD of the arithmetic by DEPTH steps of q, in slots of their own: left to itself hipcc waits
  // for each step's loads (vmcnt(0)) before it issues the next step's -- sixteen exposed round trips per workgroup,
  // on a kernel that is bound by one workgroup's critical path, not by HBM.
#ifndef PDSP_PAIRED_DEPTH2
#define PDSP_PAIRED_DEPTH2 5  /* steps of q in flight, two siblings (3: -6 %, 7: no better; tools/ab_paired.py) */
#endif
#ifndef PDSP_PAIRED_DEPTH4
#define PDSP_PAIRED_DEPTH4 2  /* four siblings, twice the registers per step (1: -4 %; 3 spills) */
#endif
  constexpr int DEPTH = P == 2 ? PDSP_PAIRED_DEPTH2 : PDSP_PAIRED_DEPTH4, SLOTS = DEPTH + 1;
  V4 l0[SLOTS][P], l1[SLOTS][P];  // planar: re / im of four points; packed: samples 8m .. 8m+3 / 8m+4 .. 8m+7
  auto issue = [&](auto qc, auto sc) {
    constexpr int q = qc, sl = sc;
    static_for<P>([&](auto pc) {
      // plain (not non-temporal) accesses on both sides: the siblings' reuse lives in the XCD's L2
      if constexpr (PK > 0) {
        // points 4m .. 4m+3 of segment p = samples 8m .. 8m+7 of the frame's half p: two 16-byte loads
        const size_t so = (size_t)t * (size_t)pk.stride + (size_t)pc * (2 * S) + 8 * (size_t)(TP * q + tid);
        l0[sl][pc] = *reinterpret_cast<const V4 *>(in_re + so);
        l1[sl][pc] = *(reinterpret_cast<const V4 *>(in_re + so) + 1);
      } else {
        const size_t o = base + (size_t)pc * S + 4 * (size_t)(TP * q + tid);
        l0[sl][pc] = *reinterpret_cast<const V4 *>(in_re + o);
        if constexpr (!REAL) l1[sl][pc] = *reinterpret_cast<const V4 *>(in_im + o);
      }
    });
  };
  static_for<DEPTH>([&](auto qc) { issue(qc, std::integral_constant<int, qc % SLOTS>{}); });
  static_for<E>([&](auto qc) {
    constexpr int q = qc, sl = q % SLOTS;
    if constexpr (q + DEPTH < E) {
      issue(std::integral_constant<int, q + DEPTH>{}, std::integral_constant<int, (q + DEPTH) % SLOTS>{});
      load_order_fence();
    }
    cx<T> x[P][4];
    static_for<P>([&](auto pc) {
      if constexpr (PK > 0) {
        V4 r0 = l0[sl][pc], r1 = l1[sl][pc];
        if constexpr (PK == 2) {
          const size_t wo = (size_t)pc * (2 * S) + 8 * (size_t)(TP * q + tid);
          r0 = r0 * *reinterpret_cast<const V4 *>(in_im + wo);
          r1 = r1 * *(reinterpret_cast<const V4 *>(in_im + wo) + 1);
        }
        if constexpr (PK >= 3) {
          cx<T> c0 = cmul(wcs, reinterpret_cast<const cx<T> *>(pk.wq)[q]);  // wave-uniform: scalar loads
          if constexpr (pc == 1) c0 = cmul(c0, wseg);
          cx<T> w[4];
          fused_window_pairs<T, PK == 4>(c0, reinterpret_cast<const cx<T> *>(pk.we), pk.k0, pk.k1, pk.k2, w);
          r0 = r0 * V4{w[0].x, w[0].y, w[1].x, w[1].y};
          r1 = r1 * V4{w[2].x, w[2].y, w[3].x, w[3].y};
        }
        x[pc][0] = cx<T>{r0.x, r0.y}, x[pc][1] = cx<T>{r0.z, r0.w}, x[pc][2] = cx<T>{r1.x, r1.y}, x[pc][3] = cx<T>{r1.z, r1.w};
      } else {
        const V4 r = l0[sl][pc];
        V4 m = V4{T(0), T(0), T(0), T(0)};
        if constexpr (!REAL) m = l1[sl][pc];
        x[pc][0] = cx<T>{r.x, m.x}, x[pc][1] = cx<T>{r.y, m.y}, x[pc][2] = cx<T>{r.z, m.z}, x[pc][3] = cx<T>{r.w, m.w};
      }
    });
    cx<T> y[4];
    static_for<4>([&](auto j) {
      if constexpr (P == 2) {
        y[j] = h ? x[0][j] - x[1][j] : x[0][j] + x[1][j];
      } else {
        // output h of the 4-point DFT over the segments: sum_p x_p (-i)^(p h)
        const cx<T> s02 = (h & 1) ? x[0][j] - x[2][j] : x[0][j] + x[2][j];
        const cx<T> s13 = (h & 1) ? x[1][j] - x[3][j] : x[1][j] + x[3][j];
        y[j] = h == 0 ? s02 + s13 : h == 2 ? s02 - s13 : h == 1 ? add_mul_neg_i(s02, s13) : add_mul_pos_i(s02, s13);
      }
    });
    if (h) {  // wave-uniform
      const cx<T> wq = look(h * 1024u * (unsigned)q);
      static_for<4>([&](auto j) { y[j] = cmul(y[j], cmul(wt[j], wq)); });
    }
    a[q] = y[0], b[q] = y[1], c[q] = y[2], d[q] = y[3];
  });

  fft_passes<T, 12, false>(a, lds, twf, tid);  // a[e] = F0[tid + TP*e]
  __syncthreads();                            // the buffer is reused by the next transform
  fft_passes<T, 12, false>(b, lds, twf, tid);
  __syncthreads();
  fft_passes<T, 12, false>(c, lds, twf, tid);
  __syncthreads();
  fft_passes<T, 12, false>(d, lds, twf, tid);

  // fft_split4_kernel's radix-4 combine; bin k of this sibling is X[P k + h]
  T *const ore = out_re + base + h, *const oim = out_im + base + h;
  auto put = [&](int k, cx<T> v) {
    v = v * scale;
    ore[(size_t)P * (size_t)(unsigned)k] = v.x;
    oim[(size_t)P * (size_t)(unsigned)k] = v.y;
  };
  static_for<E>([&](auto ec) {
    constexpr int e = ec;
    const cx<T> t1 = cmul(b[e], mul_w64<T, e>(w1));
    const cx<T> t2 = cmul(c[e], mul_w64<T, (2 * e) % 64>(w2));
    const cx<T> t3 = cmul(d[e], mul_w64<T, (3 * e) % 64>(w3));
    const cx<T> s0 = a[e] + t2, s1 = a[e] - t2, s2 = t1 + t3, d13 = t1 - t3;
    put(0 * H + TP * e + tid, s0 + s2);
    put(1 * H + TP * e + tid, add_mul_neg_i(s1, d13));
    put(2 * H + TP * e + tid, s0 - s2);
    put(3 * H + TP * e + tid, add_mul_pos_i(s1, d13));
  });
}

// The same cut one size down, as a radix-2 step: N = 8192 rows as two 4096-point transforms of the
// same 256 threads (x[2m], x[2m+1] arrive in one 2-wide load per plane) and
//   X[k] = E[k] + W_8192^k O[k],   X[k + 4096] = E[k] - W_8192^k O[k]    in registers.
// This is the f64 kernel of the largest single-pass f64 size (fft_stockham_kernel<double, 13> holds
// 139 KB of LDS, one workgroup per CU; here 69.6 KB, two), and with it the row pass of every f64
// four-step transform.   tws[k] = W_8192^k, k < 256.
template <typename T, class LD, class ST>
__global__ void __launch_bounds__(256, 2)
fft_split2_kernel(const LD ld, const ST st, const typename vec2<T>::type *__restrict__ tw12,
                  const typename vec2<T>::type *__restrict__ tws, const long long batch) {
  using TR = FftTraits<12>;
  constexpr int E = 16, TP = 256, H = 4096, N = 8192;
  static_assert(LD::kPlanar && ST::kPlanar, "planar rows");
  __shared__ cx<T> lds[TR::LROW];

  const int tid = (int)threadIdx.x;
  const long long row = uniform_row<TP>((long long)blockIdx.x);
  if (row >= batch) return;

  const cx<T> *const r2 = reinterpret_cast<const cx<T> *>(ld.plane_re() + (size_t)row * N);
  cx<T> a[E], b[E];
  // f64 complex rows: 64 data registers + 24 twiddle-base registers + the butterfly's temporaries do not
  // fit 256 VGPRs (81 spilled); reading the twiddles from the L2-resident table at each use instead
  // measured 4.36 -> 5.80 TB/s.  (f64 REAL rows no longer come here: with the bases in registers they spilled 37
  // registers in round 2's build; they run on fft_real_kernel, one 4096-point packed transform, at 6.5 TB/s.)
  constexpr bool kTableTw = sizeof(T) == 8 && LD::kHasIm;
  std::conditional_t<kTableTw, TableTwiddles<T, 12>, RegTwiddles<T, 12>> twf;
  cx<T> w1;
  if constexpr (!kTableTw) twf.load(reinterpret_cast<const cx<T> *>(tw12), tid);  // tables first
  w1 = reinterpret_cast<const cx<T> *>(tws)[(unsigned)tid];
  load_order_fence();
  if constexpr (LD::kHasIm) {
    const cx<T> *const i2 = reinterpret_cast<const cx<T> *>(ld.plane_im() + (size_t)row * N);
    static_for<E>([&](auto q) {
      const cx<T> r = ld_stream(r2 + TP * q + (unsigned)tid);
      const cx<T> m = ld_stream(i2 + TP * q + (unsigned)tid);
      a[q] = cx<T>{r.x, m.x};
      b[q] = cx<T>{r.y, m.y};
    });
  } else {
    static_for<E>([&](auto q) {
      const cx<T> r = ld_stream(r2 + TP * q + (unsigned)tid);
      a[q] = cx<T>{r.x, T(0)};
      b[q] = cx<T>{r.y, T(0)};
    });
  }
  if constexpr (kTableTw) twf.tw = reinterpret_cast<const cx<T> *>(tw12);

  fft_passes<T, 12, false>(a, lds, twf, tid);  // a[e] = E[tid + 256e]
  __syncthreads();                            // the buffer is reused by the second transform
  fft_passes<T, 12, false>(b, lds, twf, tid);  // b[e] = O[tid + 256e]

  static_for<E>([&](auto ec) {
    constexpr int e = ec;
    const cx<T> t = cmul(b[e], mul_w32<T, e>(w1));  // W_8192^(tid + 256e) = w1 * W_32^e
    st(row, TP * e, tid, a[e] + t);
    st(row, H + TP * e, tid, a[e] - t);
  });
}

}  // namespace pdsp

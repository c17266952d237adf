// pdsp_sdft_kernel.h -- the sliding DFT of rows: K chosen (fractional) bins of a window of N samples at every hop-th
// start, parallel in time and without drift (include/pdsp_hip.h, "sliding DFT").
//
// A windowed bin is 1, 3 or 5 COMPONENTS of the rectangular sliding sum X(b) = sum_{n < N} x[s + n] e^(-2 pi i b n / N)
// at fractional bins, added with real weights in registers.  Per component the row is cut into anchored chunks of N
// samples, chunk c = [cN, (c + 1)N), and with z_c[i] = x[cN + i] tab[i], tab[i] = e^(-2 pi i b i / N), i in [0, N]:
//   S_c[i]   = sum_{i' >= i} z_c[i']     (inclusive suffix scan of chunk c)
//   Pex_c[i] = sum_{i' <  i} z_c[i']     (exclusive prefix scan of chunk c)
//   X(s = cN + i) = conj(tab[i]) (S_c[i] + tab[N] Pex_{c+1}[i])
// (Van Herk / Gil-Werman): every frame is the tail of one chunk and the head of the next, so no sum is carried further
// than one chunk and frame 10^6 has the error of frame 0.  Suffixes come from a scan of their own, never as total -
// prefix: a frame's value is a function of its own N samples and of s mod N alone.
//
// THE SUMMATION ORDER (one, whatever the batch, strides, T, hop, tile or the other bins; E = 8 for f32 at N > 1024, else 4):
// a chunk is cut into rounds of B = 256 E positions, a round into 256 segments of E, segment t of round r =
// [rB + tE, rB + tE + E), one per thread; positions >= N hold zeros.
//   prefix of position i = rB + tE + e:  Pex = (RP_r + (WP_w + AP_l)) + lp_e
//     lp_e  the segment's left-to-right running sum before e: lp_0 = 0, lp_{e+1} = fma(x, tab, lp_e) per part
//     AP_l  the segment totals lp_E of the lower lanes of the wave: an inclusive Hillis-Steele scan over 64 lanes
//           (d = 1, 2, ... 32: v += v[lane - d] where lane >= d), shifted up by one lane (lane 0: 0)
//     WP_w  the lower waves' totals (the scan's value at lane 63), 0 + W_0 + ... + W_{w-1}
//     RP_r  the lower rounds' totals, 0 + R_0 + ... + R_{r-1},  R = 0 + W_0 + W_1 + W_2 + W_3  (N <= B: no RP, RS term)
//   suffix of position i:  S = (RS_r + (WS_w + AS_l)) + rs_e
//     rs_e  the segment's right-to-left running sum down to e: rs_E = 0, rs_e = fma(x, tab, rs_{e+1})
//     AS_l  the totals rs_0 of the higher lanes: the mirrored scan (v += v[lane + d] where lane + d < 64), shifted down
//     WS_w  the higher waves' totals (the scan's value at lane 0), 0 + V_3 + ... + V_{w+1}
//     RS_r  the higher rounds' totals, 0 + R_last + ... + R_{r+1}  (the R of the prefix scan of that chunk)
//   frame:  v = S + tab[N] Pex,  y = conj(tab[i]) v,  complex products as re = fma(-a.im, b.im, a.re b.re),
//           im = fma(a.im, b.re, a.re b.im);  Y = w_0 y_0, then Y = fma(w_c, y_c, Y) over the components in table order.
// Contraction is off in this header; every fused operation is written as one.
//
// One workgroup owns one bin of one row over a tile of consecutive chunks.  Per chunk c and round r it loads the round
// of chunk c (suffix role) and of chunk c + 1 (prefix role) once, runs both scans of every component in one pass over
// the wave (shuffles) and one LDS exchange of eight words, and stores the starts s = cN + i with s = 0 (mod hop) and
// s <= T - N at Y[s / hop].  Nothing is kept between chunks but the round totals R of chunk c + 1, which chunk c + 1
// needs for RS when N > B; the first chunk of a tile (or the first after a chunk without a stored start) computes its
// own R in a pass of the prefix scan alone.  Loads are clamped and selected to [0, T); a start is stored only where
// it is a frame.
#pragma once

#include "pdsp_fft_core.h"

#pragma clang fp contract(off)

namespace pdsp {

constexpr int kSdftWG = 256;
constexpr int kSdftWaves = kSdftWG / 64;
constexpr int kSdftMaxComp = 5;
constexpr int kSdftMaxRounds = 16;

template <typename T>
struct SdftWeights {
  T w[kSdftMaxComp];
};

template <typename T>
__device__ __forceinline__ T sdft_fma(const T a, const T b, const T c) {
  if constexpr (std::is_same_v<T, float>) return __builtin_fmaf(a, b, c);
  else return __builtin_fma(a, b, c);
}
// acc + x t, one rounding per part
template <typename T>
__device__ __forceinline__ cx<T> sdft_axpy(const T x, const cx<T> t, const cx<T> acc) {
  return cx<T>{sdft_fma(x, t.x, acc.x), sdft_fma(x, t.y, acc.y)};
}
template <typename T>
__device__ __forceinline__ cx<T> sdft_cmul(const cx<T> a, const cx<T> b) {
  return cx<T>{sdft_fma(-a.y, b.y, a.x * b.x), sdft_fma(a.y, b.x, a.x * b.y)};
}
template <typename T>
__device__ __forceinline__ cx<T> sdft_shfl_up(const cx<T> v, const int d) {
  return cx<T>{__shfl_up(v.x, d, 64), __shfl_up(v.y, d, 64)};
}
template <typename T>
__device__ __forceinline__ cx<T> sdft_shfl_down(const cx<T> v, const int d) {
  return cx<T>{__shfl_down(v.x, d, 64), __shfl_down(v.y, d, 64)};
}
// (The lane is made opaque at every step of the scans: the twelve comparisons are loop invariants, and hoisted out of
// the chunk loop their masks cost more scalar registers than the kernel has.)
__device__ __forceinline__ int sdft_opaque(int v) {
  asm volatile("" : "+v"(v));
  return v;
}
// inclusive scan over the lower lanes of the wave
template <typename T>
__device__ __forceinline__ cx<T> sdft_wave_prefix(cx<T> v, const int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const cx<T> u = sdft_shfl_up(v, d);
    if (sdft_opaque(lane) >= d) v = v + u;
  }
  return v;
}
// inclusive scan over the higher lanes of the wave
template <typename T>
__device__ __forceinline__ cx<T> sdft_wave_suffix(cx<T> v, const int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const cx<T> u = sdft_shfl_down(v, d);
    if (sdft_opaque(lane) + d < 64) v = v + u;
  }
  return v;
}

// How many of the E positions from i0 on lie inside the window of n positions and below `limit` (base + i0 + e <
// limit): they are the first `count`, so one comparison against a constant selects each.
template <int E>
__device__ __forceinline__ int sdft_count(const int n, const int i0, const long long g0, const long long limit) {
  long long c = limit - g0;
  if (c > n - i0) c = n - i0;
  return c < 0 ? 0 : (c > E ? E : (int)c);
}

// One round of one chunk in registers: the E samples of this thread's segment from row index g0 on, zero from `count`
// on (outside the window or the row: those are not read).
template <typename T, int E>
__device__ __forceinline__ void sdft_load(const T *x, const long long g0, const int count, T (&v)[E]) {
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const T t = x[e < count ? g0 + e : 0];
    v[e] = e < count ? t : T(0);
  }
}

template <typename T, int E>
__device__ __forceinline__ void sdft_table(const cx<T> *__restrict__ tab, const int n, const int i0, cx<T> (&tb)[E]) {
#pragma unroll
  for (int e = 0; e < E; ++e) tb[e] = tab[min(i0 + e, n)];
}

// lp[e]: the left-to-right running sum of the segment before e; returns the segment's total
template <typename T, int E>
__device__ __forceinline__ cx<T> sdft_local_prefix(const T (&x)[E], const cx<T> (&tb)[E], cx<T> (&lp)[E]) {
  cx<T> a = cx<T>{T(0), T(0)};
#pragma unroll
  for (int e = 0; e < E; ++e) {
    lp[e] = a;
    a = sdft_axpy(x[e], tb[e], a);
  }
  return a;
}

// 0 + W_0 + ... + W_{count-1}
template <typename T>
__device__ __forceinline__ cx<T> sdft_sum_up(const cx<T> *w, const int count) {
  cx<T> s = cx<T>{T(0), T(0)};
  for (int k = 0; k < count; ++k) s = s + w[k];
  return s;
}
// 0 + V_{last} + ... + V_{first}
template <typename T>
__device__ __forceinline__ cx<T> sdft_sum_down(const cx<T> *v, const int first, const int last) {
  cx<T> s = cx<T>{T(0), T(0)};
  for (int k = last; k >= first; --k) s = s + v[k];
  return s;
}

// in: `batch` rows of `samples` values at in_stride; re_out / im_out: series (row, bin) of `frames` values at
// (row nbins + bin) out_stride.  tab: per bin and component n + 1 entries.  Grid: bins fastest, then tiles, then rows.
// hop: 1 <= hop <= samples - n + 1.  The host passes min(caller's hop, samples - n + 1), which names the same starts
// (a hop beyond samples - n leaves start 0 alone); cbase + hop - 1 below is then under 2 samples and cannot overflow.
template <typename T, int E>
__global__ void __launch_bounds__(kSdftWG)
sdft_kernel(const T *__restrict__ in, const long long in_stride, const long long samples, const int n,
            const long long hop, T *__restrict__ re_out, T *__restrict__ im_out, const long long out_stride,
            const cx<T> *__restrict__ tab, const int nbins, const int ncomp, const SdftWeights<T> wts,
            const int tile_chunks, const unsigned ntiles, const long long nchunks) {
  constexpr int B = kSdftWG * E;
  __shared__ cx<T> wtot[2][2][kSdftWaves];                      // [parity][prefix / suffix][wave]
  __shared__ cx<T> rtot[2][kSdftMaxComp][kSdftMaxRounds];       // [chunk parity][component][round]

  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned bid = blockIdx.x;
  const int bin = (int)(bid % (unsigned)nbins);
  const unsigned rest = bid / (unsigned)nbins;
  const unsigned tile = rest % ntiles;
  const long long row = (long long)(rest / ntiles);

  const T *const x = in + (size_t)row * (size_t)in_stride;
  const size_t series = ((size_t)row * (size_t)nbins + (size_t)bin) * (size_t)out_stride;
  T *const ro = re_out + series;
  T *const io = im_out + series;
  const cx<T> *const tab0 = tab + (size_t)bin * (size_t)ncomp * (size_t)(n + 1);
  const int rounds = (n + B - 1) / B;
  const long long last_start = samples - n;

  long long c = (long long)tile * tile_chunks, c_end = c + tile_chunks;
  if (c_end > nchunks) c_end = nchunks;
  int par = 0;
  bool have_tot = false;  // rtot[c & 1] holds the round totals of chunk c

  for (; c < c_end; ++c) {
    const long long cbase = c * (long long)n;
    {
      // a chunk without a stored start is skipped whole (uniform)
      long long first = cbase;
      if (hop != 1) first = ((cbase + hop - 1) / hop) * hop;
      const long long hi = cbase + n - 1 < last_start ? cbase + n - 1 : last_start;
      if (first > hi) {
        have_tot = false;
        continue;
      }
    }
    if (rounds > 1 && !have_tot) {
      // the round totals of chunk c by the prefix scan alone
      for (int r = 0; r < rounds; ++r) {
        const int i0 = r * B + tid * E;
        T xs[E];
        sdft_load<T, E>(x, cbase + i0, sdft_count<E>(n, i0, cbase + i0, samples), xs);
        for (int comp = 0; comp < ncomp; ++comp) {
          cx<T> tb[E], lp[E];
          sdft_table<T, E>(tab0 + (size_t)comp * (size_t)(n + 1), n, i0, tb);
          const cx<T> a = sdft_wave_prefix<T>(sdft_local_prefix<T, E>(xs, tb, lp), lane);
          if (lane == 63) wtot[par][0][wave] = a;
          __syncthreads();
          const cx<T> total = sdft_sum_up<T>(wtot[par][0], kSdftWaves);
          if (tid == 0) rtot[c & 1][comp][r] = total;
          par ^= 1;
        }
      }
    }
    for (int r = 0; r < rounds; ++r) {
      const int i0 = r * B + tid * E;
      T xc[E], xn[E];
      const long long s0 = cbase + i0;
      sdft_load<T, E>(x, s0, sdft_count<E>(n, i0, s0, samples), xc);
      sdft_load<T, E>(x, s0 + n, sdft_count<E>(n, i0, s0 + n, samples), xn);
      cx<T> acc[E];
#pragma unroll 1
      for (int comp = 0; comp < ncomp; ++comp) {
        const cx<T> *const tc = tab0 + (size_t)comp * (size_t)(n + 1);
        cx<T> tb[E], lp[E];
        sdft_table<T, E>(tc, n, i0, tb);
        const cx<T> tabn = tc[n];
        cx<T> a = sdft_local_prefix<T, E>(xn, tb, lp);
        cx<T> b = cx<T>{T(0), T(0)};
#pragma unroll
        for (int e = E - 1; e >= 0; --e) b = sdft_axpy(xc[e], tb[e], b);
        a = sdft_wave_prefix<T>(a, lane);
        b = sdft_wave_suffix<T>(b, lane);
        if (lane == 63) wtot[par][0][wave] = a;
        if (lane == 0) wtot[par][1][wave] = b;
        __syncthreads();
        // the lower / higher lanes of this wave: the scans shifted by one lane
        cx<T> ap = sdft_shfl_up(a, 1), as = sdft_shfl_down(b, 1);
        if (lane == 0) ap = cx<T>{T(0), T(0)};
        if (lane == 63) as = cx<T>{T(0), T(0)};
        const cx<T> wp = sdft_sum_up<T>(wtot[par][0], wave);
        const cx<T> ws = sdft_sum_down<T>(wtot[par][1], wave + 1, kSdftWaves - 1);
        cx<T> pfull = wp + ap, sfull = ws + as;
        if (rounds > 1) {
          const cx<T> total = sdft_sum_up<T>(wtot[par][0], kSdftWaves);
          if (tid == 0) rtot[(c + 1) & 1][comp][r] = total;
          // R_0 ... R_{r-1} of chunk c + 1 were written in this chunk's earlier rounds, R_{r+1} ... of chunk c in the
          // previous chunk's rounds or the pass above: a barrier lies between each of those writes and these reads
          pfull = sdft_sum_up<T>(rtot[(c + 1) & 1][comp], r) + pfull;
          sfull = sdft_sum_down<T>(rtot[c & 1][comp], r + 1, rounds - 1) + sfull;
        }
        par ^= 1;
        const T w = wts.w[comp];
        cx<T> rs = cx<T>{T(0), T(0)};
#pragma unroll
        for (int e = E - 1; e >= 0; --e) {
          rs = sdft_axpy(xc[e], tb[e], rs);
          const cx<T> v = (sfull + rs) + sdft_cmul<T>(tabn, pfull + lp[e]);
          const cx<T> y = sdft_cmul<T>(cx<T>{tb[e].x, -tb[e].y}, v);
          acc[e] = comp == 0 ? cx<T>{w * y.x, w * y.y} : cx<T>{sdft_fma(w, y.x, acc[e].x), sdft_fma(w, y.y, acc[e].y)};
        }
      }
      // starts s = cbase + i0 + e that are frames: s = m hop, s <= T - N, inside the window of positions
      const int stored = sdft_count<E>(n, i0, s0, last_start + 1);
      long long m, rem;
      if (hop == 1) {
        m = s0, rem = 0;
      } else if (((unsigned long long)(s0 | hop) >> 32) == 0) {
        m = (long long)((unsigned)s0 / (unsigned)hop), rem = s0 - m * hop;
      } else {
        m = s0 / hop, rem = s0 - m * hop;
      }
#pragma unroll
      for (int e = 0; e < E; ++e) {
        if (rem == 0 && e < stored) {
          ro[m] = acc[e].x;
          io[m] = acc[e].y;
        }
        if (++rem == hop) rem = 0, ++m;
      }
    }
    have_tot = rounds > 1;
  }
}

}  // namespace pdsp

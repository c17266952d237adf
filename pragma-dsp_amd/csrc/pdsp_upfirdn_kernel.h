// pdsp_upfirdn_kernel.h -- polyphase rate change of real rows in the time domain (scipy.signal.upfirdn, and
// scipy.signal.resample_poly on top of it): upsample by `up` (zero stuffing), filter with `ntaps` real taps, keep
// every `down`-th sample from offset t0 on -- without the stuffed zeros or the discarded outputs ever existing:
//   y[m] = sum_k h[m down + t0 - k up] x[k],   0 <= k < len, 0 <= tap index < ntaps.
// With q = m down + t0, phase p = q mod up and base k0 = q div up this is
//   y[m] = sum_{j = 0}^{T - 1} g[p][j] x[k0 - j],   g[p][j] = h[p + j up],   T = ceil(ntaps / up),
// x read as 0 outside [0, len), g zero-padded: the host reorders the taps once per resampler into the phase-major table
// g (`up` rows of T).  Every output is summed j ascending, one fma per term, from +0: its value depends on the taps and
// the samples alone, not on the tile it falls in, the batch or the row's placement (padding terms add a zero product,
// which leaves any accumulator as it is).
//
// One workgroup computes `up * bper` consecutive outputs of one row (a tile): it stages the taps (row stride `tp`,
// odd where LDS has room, so that lanes on different phases read different banks) and the tile's input span, loaded
// once with zero fill, and then runs work items.  An item is R outputs of ONE phase, m = m0 + up b for R values of b:
// they share the T taps, which the item reads once each into a register.  Per output that is T / R tap reads and
//   WIN = false: T sample reads; the item's b are bper / R apart, so adjacent lanes hold adjacent outputs (coalesced
//                stores, sample reads `down / up` apart from lane to lane);
//   WIN = true:  down == 1 only.  The item's b are consecutive, so its R outputs read a sliding window of the samples:
//                the window lives in R registers and takes ONE new sample per tap: 2 T / R LDS reads per output.
// The tile origin (m0 down + t0, its phase and base) is computed once in 64 bits; everything inside a tile is 32-bit
// (the host bounds the span, hence every in-tile product: pdsp_kernels_resample.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace pdsp {

constexpr int kUpfirdnWG = 256;
constexpr int kUpfirdnFront = 8;  // zero samples in front of the span: WIN's window reads up to R past the last tap

// x: rows of `len` samples at x_stride; y: rows of y_len outputs at y_stride; g: up * tn taps, phase-major;
// span: samples staged per tile (>= what any phase origin needs); tiles: tiles per row.  Dynamic LDS:
// (up * tp + kUpfirdnFront + span) values (GT: without the taps).
//   GT: the taps stay in global memory (g, row stride tn) and LDS holds samples only: the fallback for tap tables that
//       leave no room for a tile's span (up and ntaps both in the thousands, f64).
template <typename T, int R, bool WIN, bool GT>
__global__ void __launch_bounds__(kUpfirdnWG)
upfirdn_kernel(const T *__restrict__ xin, const long long len, const long long x_stride, const T *__restrict__ g,
               const int up, const int down, const int t0, const int tn, const int tp, T *__restrict__ yout,
               const long long y_len, const long long y_stride, const int bper, const int span, const unsigned tiles) {
  static_assert(!WIN || R <= kUpfirdnFront, "the front padding covers WIN's window");
  extern __shared__ __align__(16) unsigned char upfirdn_lds[];
  T *const gl = reinterpret_cast<T *>(upfirdn_lds);
  T *const xl = gl + (GT ? 0 : up * tp) + kUpfirdnFront;

  const int tid = threadIdx.x;
  const unsigned row = blockIdx.x / tiles, tile = blockIdx.x - row * tiles;
  const int tile_out = up * bper;
  const long long m_tile = (long long)tile * tile_out;
  const long long q_lo = m_tile * down + t0;
  const long long k_lo = q_lo / up;
  const int p_lo = (int)(q_lo - k_lo * up);
  const long long xs0 = k_lo - (tn - 1);  // the row index of xl[0]

  if constexpr (!GT) {
    for (int e = tid; e < up * tn; e += kUpfirdnWG) {
      const int p = e / tn;
      gl[p * tp + (e - p * tn)] = g[e];
    }
  }
  if (tid < kUpfirdnFront) xl[-1 - tid] = T(0);
  {
    const T *const xrow = xin + (long long)row * x_stride;
    const long long lo64 = -xs0, hi64 = len - xs0;
    const int lo = lo64 < 0 ? 0 : (lo64 > span ? span : (int)lo64);
    const int hi = hi64 < 0 ? 0 : (hi64 > span ? span : (int)hi64);
    for (int e = tid; e < span; e += kUpfirdnWG) {
      T v = T(0);
      if (e >= lo && e < hi) v = xrow[xs0 + e];
      xl[e] = v;
    }
  }
  __syncthreads();

  const long long left = y_len - m_tile;
  const int o_lim = left < tile_out ? (int)left : tile_out;
  T *const yrow = yout + (long long)row * y_stride + m_tile;
  const int groups = bper / R;
  for (int w = tid; w < up * groups; w += kUpfirdnWG) {
    const int bg = w / up, a = w - bg * up;
    const int qa = p_lo + a * down;
    const int ka = qa / up, p = qa - ka * up;
    const T *const gp = GT ? g + p * tn : gl + p * tp;
    T acc[R];
#pragma unroll
    for (int i = 0; i < R; ++i) acc[i] = T(0);
    if constexpr (WIN) {
      // outputs b = bg R + i: sample of (i, j) is xp[i - j]; v[(i - jj) mod R] holds it at step j = jb + jj
      const T *const xp = xl + ka + bg * R + (tn - 1);
      T v[R];
#pragma unroll
      for (int i = 0; i < R; ++i) v[i] = xp[i];
      for (int jb = 0; jb < tn; jb += R) {
#pragma unroll
        for (int jj = 0; jj < R; ++jj) {
          const int j = jb + jj;
          const T tap = j < tn ? gp[j] : T(0);
#pragma unroll
          for (int i = 0; i < R; ++i) acc[i] = fma(tap, v[(i - jj + R) % R], acc[i]);
          v[(R - 1 - jj) % R] = xp[-(j + 1)];
        }
      }
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const int o = a + up * (bg * R + i);
        if (o < o_lim) yrow[o] = acc[i];
      }
    } else {
      // outputs b = bg + i groups: sample of (i, j) is xp[i xstep - j]
      const int xstep = groups * down;
      const T *const xp = xl + ka + bg * down + (tn - 1);
#pragma unroll 4
      for (int j = 0; j < tn; ++j) {
        const T tap = gp[j];
#pragma unroll
        for (int i = 0; i < R; ++i) acc[i] = fma(tap, xp[i * xstep - j], acc[i]);
      }
#pragma unroll
      for (int i = 0; i < R; ++i) {
        const int o = a + up * (bg + i * groups);
        if (o < o_lim) yrow[o] = acc[i];
      }
    }
  }
}

}  // namespace pdsp

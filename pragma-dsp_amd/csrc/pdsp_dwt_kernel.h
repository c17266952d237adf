// pdsp_dwt_kernel.h -- the multi-level discrete wavelet transform of real rows (wavedec / waverec) with an orthogonal
// filter pair and periodic extension, every call one launch.  h: the scaling filter, F taps (even, 2 ... 32);
// g[j] = (-1)^j h[F - 1 - j].  One analysis level on a row a of even length m:
//   cA[k] = sum_j h[j] a[(2k + j) mod m],   cD[k] = sum_j g[j] a[(2k + j) mod m],   0 <= k < m / 2,
// and its inverse, the transpose, for the output pair (2i, 2i + 1), m' = m / 2:
//   x[2i]     = sum_t h[2t]     cA[(i - t) mod m'] + g[2t]     cD[(i - t) mod m'],
//   x[2i + 1] = sum_t h[2t + 1] cA[(i - t) mod m'] + g[2t + 1] cD[(i - t) mod m'],   0 <= t < F / 2.
// J levels give the Mallat layout [cA_J | cD_J | cD_{J-1} | ... | cD_1] in one row of n = len values (n mod 2^J = 0).
// Every value is summed in one fixed order -- forward: j ascending; inverse: t ascending, the cA term before the cD
// term -- one fma per term from +0, by dwt_analysis() / dwt_synthesis() below on every path: its bits depend on the
// taps and the samples alone, not on the path, the tile, the batch or the row's placement.
//
// Two paths per direction (RES), chosen by the host (pdsp_kernels_dwt.hip):
//   RES = true:  one workgroup per row; the whole row is loaded into LDS before anything is stored (the exact in-place
//                call is legal) and all J levels run there with modular indexing: no halo, any J down to a last level
//                of length 2.
//   RES = false: a workgroup owns `tile` consecutive positions of a row (a multiple of 2^J) and every coefficient (the
//                inverse: every sample) they produce.  The forward stages tile + (F - 2)(2^J - 1) samples, wrapped
//                round the row on load -- as often as the span is long -- and each level computes the approximation
//                over its shrinking halo, (F - 2)(2^(J-l) - 1) at level l.  The inverse stages, level by level, the
//                band's coefficients with F - 2 of them in front of the tile.  Nothing inside a tile wraps.
// An approximation row in LDS lies de-interleaved by parity (even samples, then odd), so that lanes on adjacent k read
// E[k + j / 2] and O[k + j / 2] at unit stride.  The taps (h, then g: 2F values of T) are uniform across lanes and are
// read from their global table with scalar loads.  row * stride and tile origins are 64-bit; every index inside a
// tile is 32-bit (the host bounds the spans).
#pragma once
#include <hip/hip_runtime.h>

namespace pdsp {

constexpr int kDwtWG = 256;

// cA and cD of one output from the same sample reads: E / O are the even / odd samples of the level's input, q the
// index of the pair (2k, 2k + 1), `wrap` the pairs per period (beyond any index where nothing wraps).
template <typename T>
__device__ __forceinline__ void dwt_analysis(const T *__restrict__ hg, const int f, const T *e, const T *o, int q,
                                             const int wrap, T &ca, T &cd) {
  ca = T(0), cd = T(0);
  for (int j = 0; j < f; j += 2) {
    const T ve = e[q], vo = o[q];
    ca = fma(hg[j], ve, ca);
    cd = fma(hg[f + j], ve, cd);
    ca = fma(hg[j + 1], vo, ca);
    cd = fma(hg[f + j + 1], vo, cd);
    if (++q == wrap) q = 0;
  }
}

// x[2i] and x[2i + 1] from the same coefficient reads: q the index of (cA, cD)[i], `back` the index that follows
// index 0 (m' - 1; unused where nothing wraps).
template <typename T>
__device__ __forceinline__ void dwt_synthesis(const T *__restrict__ hg, const int f, const T *ca, const T *cd, int q,
                                              const int back, T &x0, T &x1) {
  x0 = T(0), x1 = T(0);
  for (int j = 0; j < f; j += 2) {
    const T va = ca[q], vd = cd[q];
    x0 = fma(hg[j], va, x0);
    x1 = fma(hg[j + 1], va, x1);
    x0 = fma(hg[f + j], vd, x0);
    x1 = fma(hg[f + j + 1], vd, x1);
    q = q == 0 ? back : q - 1;
  }
}

// x: rows of len samples at x_stride; y: rows of len coefficients at y_stride; hg: h | g.  tile: positions per
// workgroup (RES: len), halo = (f - 2)(2^levels - 1) (RES: 0), tiles per row (RES: 1).  Dynamic LDS:
// L0 + L1 values, L0 = tile + halo, L1 = (L0 - (f - 2)) / 2 (RES: len / 2).
template <typename T, bool RES>
__global__ void __launch_bounds__(kDwtWG)
dwt_forward_kernel(const T *__restrict__ xin, const long long len, const long long x_stride, const T *__restrict__ hg,
                   const int f, const int levels, T *__restrict__ yout, const long long y_stride, const int tile,
                   const int halo, const unsigned tiles) {
  extern __shared__ __align__(16) unsigned char dwt_lds[];
  const int tid = threadIdx.x;
  const unsigned row = blockIdx.x / tiles, t = blockIdx.x - row * tiles;
  const long long t0 = (long long)t * tile;
  const long long left = len - t0;
  const int own = left < tile ? (int)left : tile;  // a multiple of 2^levels, as len and tile are
  int lin = own + halo;
  T *src = reinterpret_cast<T *>(dwt_lds);
  T *dst = src + (tile + halo);

  {
    const T *const xrow = xin + (long long)row * x_stride;
    const int half = lin >> 1;
    for (int e = tid; e < lin; e += kDwtWG) {
      long long p = t0 + e;
      if constexpr (!RES)
        if (p >= len) p %= len;
      src[(e & 1) * half + (e >> 1)] = xrow[p];
    }
  }
  __syncthreads();

  T *const yrow = yout + (long long)row * y_stride;
  for (int l = 1; l <= levels; ++l) {
    const int half = lin >> 1;
    const int lout = RES ? half : (lin - (f - 2)) >> 1;
    const int owned = own >> l;
    const long long m = len >> l, base = t0 >> l;
    const int ohalf = lout >> 1;
    for (int i = tid; i < lout; i += kDwtWG) {
      T ca, cd;
      dwt_analysis(hg, f, src, src + half, i, RES ? half : 0x7fffffff, ca, cd);
      if (i < owned) yrow[m + base + i] = cd;
      if (l == levels) {
        if (i < owned) yrow[base + i] = ca;
      } else {
        dst[(i & 1) * ohalf + (i >> 1)] = ca;
      }
    }
    __syncthreads();
    T *const s = src;
    src = dst, dst = s;
    lin = lout;
  }
}

// c: rows of len coefficients at c_stride; x: rows of len samples at x_stride.  tile, tiles as above; the halo in
// front of a tile is f - 2 coefficients of every band (RES: none).  Dynamic LDS, in values:
//   RES:  len (the row) + len / 2 + len / 4 (the approximations of odd / even level);
//   else: 3 (f - 2) + tile / 2 (a band's details) + tile / 2 + tile / 4.
template <typename T, bool RES>
__global__ void __launch_bounds__(kDwtWG)
dwt_inverse_kernel(const T *__restrict__ cin, const long long len, const long long c_stride, const T *__restrict__ hg,
                   const int f, const int levels, T *__restrict__ xout, const long long x_stride, const int tile,
                   const unsigned tiles) {
  extern __shared__ __align__(16) unsigned char dwt_lds[];
  const int tid = threadIdx.x;
  const unsigned row = blockIdx.x / tiles, t = blockIdx.x - row * tiles;
  const long long t0 = (long long)t * tile;
  const long long left = len - t0;
  const int own = left < tile ? (int)left : tile;
  const int g = RES ? 0 : f - 2;
  const T *const crow = cin + (long long)row * c_stride;

  // det: the row (RES) or the current band's details; odd / even: the approximation of an odd / even level
  T *const det = reinterpret_cast<T *>(dwt_lds);
  T *const odd = det + (RES ? tile : (tile >> 1) + g);
  T *const even = odd + (tile >> 1) + g;

  const T *ca;
  if constexpr (RES) {
    for (int e = tid; e < own; e += kDwtWG) det[e] = crow[e];
    ca = det;
  } else {
    const long long m = len >> levels;
    long long b = ((t0 >> levels) - g) % m;
    if (b < 0) b += m;
    T *const a = (levels & 1) ? odd : even;
    const int la = (own >> levels) + g;
    for (int e = tid; e < la; e += kDwtWG) {
      long long p = b + e;
      if (p >= m) p %= m;
      a[e] = crow[p];
    }
    ca = a;
  }

  T *const xrow = xout + (long long)row * x_stride + t0;
  for (int l = levels; l >= 1; --l) {
    const long long m = len >> l;
    const T *cd;
    if constexpr (RES) {
      cd = det + (int)m;
      __syncthreads();
    } else {
      long long b = ((t0 >> l) - g) % m;
      if (b < 0) b += m;
      const int la = (own >> l) + g;
      for (int e = tid; e < la; e += kDwtWG) {
        long long p = b + e;
        if (p >= m) p %= m;
        det[e] = crow[m + p];
      }
      cd = det;
      __syncthreads();
    }
    const int gout = l == 1 ? 0 : g;                // the halo in front of the level's output
    const int pairs = ((own >> (l - 1)) + gout) >> 1;
    const int shift = g - (gout >> 1);              // pair u reads the coefficients from index u + shift down
    T *const out = ((l - 1) & 1) ? odd : even;
    for (int u = tid; u < pairs; u += kDwtWG) {
      T x0, x1;
      dwt_synthesis(hg, f, ca, cd, u + shift, RES ? (int)m - 1 : 0, x0, x1);
      if (l == 1) {
        xrow[2 * u] = x0, xrow[2 * u + 1] = x1;
      } else {
        out[2 * u] = x0, out[2 * u + 1] = x1;
      }
    }
    __syncthreads();  // the tiled path overwrites det next
    ca = out;
  }
}

}  // namespace pdsp

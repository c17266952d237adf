// Kernel unit: the sliding DFT of rows (pdsp_sdft_kernel.h), f32 and f64.
// See pdsp_internal.h.  The callers in pdsp_capi_sdft.hip have validated every argument.
#include <cstdlib>

#include "pdsp_internal.h"
#include "pdsp_sdft_kernel.h"

namespace pdsp_host {

// Chunks per workgroup.  A tile's first chunk costs one extra prefix scan where N > 256 E; below that a tile carries
// nothing, and the default only sizes the work of a workgroup.  PDSP_SDFT_TILE_CHUNKS (read at the call, like
// PDSP_HOST_THREADS) forces small tiles for tests; the bits do not depend on it.
int sdft_tile_chunks(long long n, size_t elem) {
  if (const char *e = getenv("PDSP_SDFT_TILE_CHUNKS")) {
    const long v = atol(e);
    if (v >= 1 && v <= 1 << 20) return (int)v;
  }
  return n > 256LL * sdft_segment(n, elem) ? 8 : 16;
}

long long sdft_blocks(long long n, size_t elem, long long samples, long long nbins, long long batch) {
  const long long nchunks = (samples - n) / n + 1, tc = sdft_tile_chunks(n, elem), ntiles = (nchunks + tc - 1) / tc;
  long long b = 0;
  if (__builtin_mul_overflow(ntiles, nbins, &b) || __builtin_mul_overflow(b, batch, &b)) return -1;
  return b;
}

template <typename T>
int sdft_dev(long long n, long long hop, int nbins, int ncomp, const double *weights, long long batch, const T *in,
             long long in_stride, long long samples, T *re_out, T *im_out, long long out_stride,
             const typename pdsp::vec2<T>::type *tab, hipStream_t s) {
  const long long nchunks = (samples - n) / n + 1, tc = sdft_tile_chunks(n, sizeof(T)), ntiles = (nchunks + tc - 1) / tc;
  const long long blocks = ntiles * nbins * batch;
  pdsp::SdftWeights<T> w{};
  for (int i = 0; i < ncomp; ++i) w.w[i] = (T)weights[i];
  // The kernel's hop is min(hop, T - N + 1).  The starts are the multiples of hop up to T - N: a hop beyond T - N
  // leaves start 0 alone, as T - N + 1 does, and any smaller hop is passed as it is.  The kernel rounds a chunk's base
  // up to a multiple of its hop in 64 bits; with hop <= T - N + 1 that sum stays below 2 T (the caller's hop has no
  // upper limit, and cbase + hop overflowed from 2^63 - cbase on).  Frame counts and pdsp_sdft_hop keep the caller's.
  const long long khop = hop < samples - n + 1 ? hop : samples - n + 1;
  const auto go = [&](auto e) {
    constexpr int E = decltype(e)::value;
    hipLaunchKernelGGL((pdsp::sdft_kernel<T, E>), dim3((unsigned)blocks), dim3(pdsp::kSdftWG), 0, s, in, in_stride,
                       samples, (int)n, khop, re_out, im_out, out_stride, reinterpret_cast<const pdsp::cx<T> *>(tab),
                       nbins, ncomp, w, (int)tc, (unsigned)ntiles, nchunks);
    return hipGetLastError();
  };
  hipError_t e = hipSuccess;
  if constexpr (sizeof(T) == 4) e = sdft_segment(n, 4) == 4 ? go(int_c<4>{}) : go(int_c<8>{});
  else e = go(int_c<4>{});
  PDSP_HIP_TRY(e);
  return PDSP_OK;
}

template int sdft_dev<float>(long long, long long, int, int, const double *, long long, const float *, long long,
                             long long, float *, float *, long long, const float2 *, hipStream_t);
template int sdft_dev<double>(long long, long long, int, int, const double *, long long, const double *, long long,
                              long long, double *, double *, long long, const double2 *, hipStream_t);

}  // namespace pdsp_host

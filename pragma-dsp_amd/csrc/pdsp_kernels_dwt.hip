// Kernel unit: the multi-level wavelet transform of real rows (pdsp_dwt_kernel.h), f32 and f64, and the rule that
// chooses the path and sizes a tile.  See pdsp_internal.h.  The callers in pdsp_capi_dwt.hip have validated every argument.
#include "pdsp_internal.h"
#include "pdsp_dwt_kernel.h"

namespace pdsp_host {

int g_dwt_tile = 0;  // pdsp_set_dwt_tile: 0 = the rule below

// The tile rule, in values of `elem` bytes; F taps, J levels, rows of n.
//   resident: forward n + n / 2, inverse n + n / 2 + n / 4 values of LDS.  Taken when that is at most 64 KiB (two or
//             more rows per CU), and up to 160 KiB when the tiled path refuses the depth.
//   tiled:    T positions per workgroup, a multiple of 2^J: 4096 (f32) / 2048 (f64) rounded down to one, at least 2^J,
//             the forward at least its halo (F - 2)(2^J - 1) rounded up to one; never more than the row.  LDS: forward
//             (T + halo) + (T + halo - (F - 2)) / 2, inverse 5 T / 4 + 3 (F - 2).  The depth limit
//             max(halo, 2^J) <= 32 KiB of values (8192 f32, 4096 f64), the inverse's halo being F - 2, keeps every
//             tile within 96 KiB.
// g_dwt_tile (development, pdsp_hip_dev.h): bits 0-1 force the resident (1) or the tiled (2) path, the rest caps T
// (rounded up to a multiple of 2^J).  A forced path is never replaced: false where it does not fit.
bool dwt_tile(long long f, long long levels, long long n, size_t elem, bool inverse, DwtTile *out, long long *limit) {
  const long long e_small = 65536 / (long long)elem, e_max = 163840 / (long long)elem, e_halo = 32768 / (long long)elem;
  const int forced = g_dwt_tile & 3;
  const long long cap = g_dwt_tile >> 2;
  const long long res = inverse ? n + n / 2 + n / 4 : n + n / 2;
  *limit = e_halo;
  DwtTile t;
  auto resident = [&] {
    t.resident = true, t.tile = n, t.halo = 0, t.tiles = 1, t.lds_bytes = (size_t)res * elem;
    return *out = t, true;
  };
  const bool deep = levels >= 62;  // 2^levels beyond any row the tiled path takes
  const long long step = deep ? 0 : 1LL << levels;
  const long long halo = deep ? 0 : (inverse ? f - 2 : (f - 2) * (step - 1));
  const bool tiled_ok = !deep && step <= e_halo && halo <= e_halo;
  if (forced == 1) return res <= e_max && resident();
  if (forced == 0 && (res <= e_small || (!tiled_ok && res <= e_max))) return resident();
  if (!tiled_ok) return false;
  long long tile = (elem == 4 ? 4096 : 2048) / step * step;
  if (tile < step) tile = step;
  if (!inverse && tile < halo) tile = (halo + step - 1) / step * step;
  if (tile > n) tile = n;
  if (cap > 0 && tile > (cap + step - 1) / step * step) tile = (cap + step - 1) / step * step;
  t.resident = false, t.tile = tile, t.halo = halo, t.tiles = (n + tile - 1) / tile;
  const long long values = inverse ? tile / 2 + tile / 2 + tile / 4 + 3 * halo : (tile + halo) + (tile + halo - (f - 2)) / 2;
  t.lds_bytes = (size_t)values * elem;
  return *out = t, true;
}

// the deepest forward transform the tiled path takes: max((F - 2)(2^J - 1), 2^J) <= 32 KiB of values
int dwt_tiled_max_levels(long long f, size_t elem) {
  const long long limit = 32768 / (long long)elem;
  int most = 0;
  while ((1LL << (most + 1)) <= limit && (f - 2) * ((1LL << (most + 1)) - 1) <= limit) ++most;
  return most;
}

int dwt_tile_checked(long long f, long long levels, long long n, size_t elem, bool inverse, DwtTile *out) {
  long long limit = 0;
  if (dwt_tile(f, levels, n, elem, inverse, out, &limit)) return PDSP_OK;
  if ((g_dwt_tile & 3) == 1)
    return fail(PDSP_ERR_UNSUPPORTED_SIZE, "the forced resident path has no room for rows of %lld values of %zu bytes in "
                "160 KiB of LDS (pdsp_set_dwt_tile)", n, elem);
  if (inverse)
    return fail(PDSP_ERR_UNSUPPORTED_SIZE, "inverse DWT of %lld levels on rows of %lld: beyond the resident path a tile is "
                "a multiple of 2^levels, at most %lld values", levels, n, limit);
  const int most = dwt_tiled_max_levels(f, elem);
  return fail(PDSP_ERR_UNSUPPORTED_SIZE, "forward DWT of %lld levels with %lld taps on rows of %lld: beyond the resident "
              "path max(halo, 2^levels) must be <= %lld values, halo = (taps - 2)(2^levels - 1): at most %d levels",
              levels, f, n, limit, most);
}

template <typename T, bool RES, bool INV>
static hipError_t dwt_launch(const DwtTile &t, unsigned blocks, const T *hg, int f, int levels, const T *in,
                             long long len, long long in_stride, T *out, long long out_stride, hipStream_t s) {
  if constexpr (INV) {
    auto *const k = &pdsp::dwt_inverse_kernel<T, RES>;
    if (t.lds_bytes > 65536)  // beyond the default limit of dynamic LDS
      if (hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, 163840))
        return e;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(pdsp::kDwtWG), t.lds_bytes, s, in, len, in_stride, hg, f, levels, out,
                       out_stride, (int)t.tile, (unsigned)t.tiles);
  } else {
    auto *const k = &pdsp::dwt_forward_kernel<T, RES>;
    if (t.lds_bytes > 65536)
      if (hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, 163840))
        return e;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(pdsp::kDwtWG), t.lds_bytes, s, in, len, in_stride, hg, f, levels, out,
                       out_stride, (int)t.tile, (int)t.halo, (unsigned)t.tiles);
  }
  return hipGetLastError();
}

template <typename T>
int dwt_dev(const DwtTile &t, const T *hg, int f, int levels, bool inverse, long long batch, const T *in, long long len,
            long long in_stride, T *out, long long out_stride, hipStream_t s) {
  const unsigned blocks = (unsigned)(batch * t.tiles);  // the caller has bounded the product
  const hipError_t e =
      inverse ? (t.resident ? dwt_launch<T, true, true>(t, blocks, hg, f, levels, in, len, in_stride, out, out_stride, s)
                            : dwt_launch<T, false, true>(t, blocks, hg, f, levels, in, len, in_stride, out, out_stride, s))
              : (t.resident ? dwt_launch<T, true, false>(t, blocks, hg, f, levels, in, len, in_stride, out, out_stride, s)
                            : dwt_launch<T, false, false>(t, blocks, hg, f, levels, in, len, in_stride, out, out_stride, s));
  PDSP_HIP_TRY(e);
  return PDSP_OK;
}

template int dwt_dev<float>(const DwtTile &, const float *, int, int, bool, long long, const float *, long long,
                            long long, float *, long long, hipStream_t);
template int dwt_dev<double>(const DwtTile &, const double *, int, int, bool, long long, const double *, long long,
                             long long, double *, long long, hipStream_t);

}  // namespace pdsp_host

// Kernel unit: polyphase rate change of real rows (pdsp_upfirdn_kernel.h), f32 and f64, and the rule that sizes a
// tile.  See pdsp_internal.h.  The callers in pdsp_capi_resample.hip have validated every argument.
#include "pdsp_internal.h"
#include "pdsp_upfirdn_kernel.h"

namespace pdsp_host {

int g_upfirdn_tile = 0;  // pdsp_set_upfirdn_tile: 0 = the rule below

// The tile rule.  T = ceil(ntaps / up) taps per phase; a tile is up * B consecutive outputs, B a
// multiple of R; LDS holds up * tp taps + kUpfirdnFront + span samples, span = T + floor((up - 1 + (up B - 1) down) / up)
// (the worst phase origin).  B starts at R ceil(4 * 256 / up) -- four items per thread -- capped by the row's outputs;
// it is halved while the tile exceeds 64 KiB and would still leave every thread an item, then while it exceeds
// 160 KiB.  R: 8 with the sliding window when down == 1, else 4; 1 when that leaves a tile fewer than 64 items (long
// filters at high decimation: more, smaller items) or does not fit; and when the tap table leaves no room for a span
// (up * T and down both near 8192, f64), R = 1 with the taps read from global memory.
// g_upfirdn_tile (development, pdsp_hip_dev.h) caps B and / or forces one instantiation, which then is the only
// candidate: false where it is not legal for the call or does not fit.
bool upfirdn_tile(long long up, long long down, long long ntaps, long long y_len, size_t elem, UpfirdnTile *out) {
  constexpr long long WG = pdsp::kUpfirdnWG, FRONT = pdsp::kUpfirdnFront;
  const long long tn = (ntaps + up - 1) / up;
  const long long e_small = 65536 / (long long)elem, e_max = 163840 / (long long)elem;
  const int forced = g_upfirdn_tile & 15;
  const long long cap = g_upfirdn_tile >> 4;
  auto fit = [&](long long r, bool win, bool gt, UpfirdnTile *t) {
    long long tp = (up > 1 && tn % 2 == 0) ? tn + 1 : tn;
    auto entries = [&](long long b) { return (gt ? 0 : up * tp) + FRONT + tn + (up - 1 + (up * b - 1) * down) / up; };
    if (entries(r) > e_max) tp = tn;
    long long b = r * ((4 * WG + up - 1) / up);
    const long long by = (((y_len + up - 1) / up + r - 1) / r) * r;
    if (b > by) b = by;
    if (cap > 0 && b > ((cap + r - 1) / r) * r) b = ((cap + r - 1) / r) * r;
    auto half = [&](long long v) { return ((v / 2 + r - 1) / r) * r; };
    while (entries(b) > e_small && b > r && up * (half(b) / r) >= WG) b = half(b);
    while (entries(b) > e_max && b > r) b = half(b);
    if (entries(b) > e_max) return false;
    t->r = (int)r, t->win = win, t->gt = gt, t->tn = (int)tn, t->tp = (int)tp, t->bper = (int)b;
    t->span = (int)(entries(b) - (gt ? 0 : up * tp) - FRONT);
    t->lds_bytes = (size_t)entries(b) * elem;
    t->items = up * (b / r);
    return true;
  };
  if (forced == 1) return fit(4, false, false, out);
  if (forced == 2) return down == 1 && fit(8, true, false, out);
  if (forced == 3) return fit(1, false, false, out);
  if (forced == 4) return fit(1, false, true, out);
  UpfirdnTile pref, one;
  const bool have_pref = down == 1 ? fit(8, true, false, &pref) : fit(4, false, false, &pref);
  if (have_pref && pref.items >= 64) return *out = pref, true;
  if (fit(1, false, false, &one)) return *out = one, true;
  if (have_pref) return *out = pref, true;
  return fit(1, false, true, out);  // the taps stay in global memory: the span alone always fits
}

int upfirdn_tile_checked(long long up, long long down, long long ntaps, long long y_len, size_t elem, UpfirdnTile *out) {
  if (upfirdn_tile(up, down, ntaps, y_len, elem, out)) return PDSP_OK;
  static const char *const kName[5] = {"", "R = 4", "R = 8, WIN", "R = 1", "R = 1, GT"};
  if (const int forced = g_upfirdn_tile & 15)
    return fail(PDSP_ERR_UNSUPPORTED_SIZE,
                "the forced instantiation (%s) %s up %lld, down %lld, %lld taps of %zu bytes (pdsp_set_upfirdn_tile)",
                kName[forced], forced == 2 && down != 1 ? "needs down == 1: got" : "has no tile within 160 KiB of LDS for",
                up, down, ntaps, elem);
  return fail(PDSP_ERR_UNSUPPORTED_SIZE, "no tile of up %lld, down %lld, %lld taps fits LDS", up, down, ntaps);
}

template <typename T, int R, bool WIN, bool GT>
static hipError_t upfirdn_launch(const UpfirdnTile &t, unsigned blocks, unsigned tiles, const T *g, int up, int down,
                                 int t0, const T *x, long long len, long long x_stride, T *y, long long y_len,
                                 long long y_stride, hipStream_t s) {
  auto *const k = &pdsp::upfirdn_kernel<T, R, WIN, GT>;
  if (t.lds_bytes > 65536)  // beyond the default limit of dynamic LDS
    if (hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, 163840))
      return e;
  hipLaunchKernelGGL(k, dim3(blocks), dim3(pdsp::kUpfirdnWG), t.lds_bytes, s, x, len, x_stride, g, up, down, t0, t.tn,
                     t.tp, y, y_len, y_stride, t.bper, t.span, tiles);
  return hipGetLastError();
}

template <typename T>
int upfirdn_dev(const T *g, long long up, long long down, long long ntaps, long long t0, long long batch, const T *x,
                long long len, long long x_stride, T *y, long long y_len, long long y_stride, hipStream_t s) {
  UpfirdnTile t;
  if (int rc = upfirdn_tile_checked(up, down, ntaps, y_len, sizeof(T), &t)) return rc;
  const long long tile_out = up * t.bper, tiles = (y_len + tile_out - 1) / tile_out;
  long long blocks = 0;
  if (__builtin_mul_overflow(batch, tiles, &blocks) || blocks > 0x7fffffffLL)
    return fail(PDSP_ERR_BAD_ARG, "batch too large: %lld rows of %lld tiles", batch, tiles);
  auto go = [&](auto r, auto win, auto gt) {
    return upfirdn_launch<T, decltype(r)::value, decltype(win)::value, decltype(gt)::value>(
        t, (unsigned)blocks, (unsigned)tiles, g, (int)up, (int)down, (int)t0, x, len, x_stride, y, y_len, y_stride, s);
  };
  const std::true_type yes;
  const std::false_type no;
  const hipError_t e = t.win      ? go(int_c<8>{}, yes, no)
                       : t.r == 4 ? go(int_c<4>{}, no, no)
                       : t.gt     ? go(int_c<1>{}, no, yes)
                                  : go(int_c<1>{}, no, no);
  PDSP_HIP_TRY(e);
  return PDSP_OK;
}

template int upfirdn_dev<float>(const float *, long long, long long, long long, long long, long long, const float *,
                                long long, long long, float *, long long, long long, hipStream_t);
template int upfirdn_dev<double>(const double *, long long, long long, long long, long long, long long, const double *,
                                 long long, long long, double *, long long, long long, hipStream_t);

}  // namespace pdsp_host

// pdsp_capi_dwt.hip -- the multi-level wavelet transform (wavedec / waverec): the Daubechies table, the handle, entry points, host forms.
// Host side only; calls dwt_dev, dwt_tile_checked and dwt_tiled_max_levels (pdsp_kernels_dwt.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "pdsp_host.h"

using namespace pdsp_host;

/* ---- multi-level wavelet transform: wavedec / waverec -------------------------- */

// A wavelet transform is its scaling filter and its depth: no FFT size, so no plan.  The taps are kept in f64, h | g,
// rounded once per precision and uploaded on first use (TableHandle, first_use_table).
struct pdsp_dwt : TableHandle {
  int levels = 1;
  std::vector<double> hg;  // h | g, g[j] = (-1)^j h[F - 1 - j]
  float *hg32 = nullptr;
  double *hg64 = nullptr;
  template <typename T>
  auto &slot() {
    if constexpr (sizeof(T) == 4) return hg32;
    else return hg64;
  }
};

namespace {

constexpr long long kDwtMaxTaps = 32;
constexpr int kDaubechiesMax = 10;
// Daubechies' extremal-phase scaling filters db1 ... db10, sum sqrt 2 (tools/gen_daubechies.py prints this table)
const double kDaubechies[] = {
    // db1
    0.7071067811865476, 0.7071067811865476,
    // db2
    0.48296291314453427, 0.836516303737808, 0.22414386804201333, -0.12940952255126045,
    // db3
    0.3326705529500826, 0.8068915093110924, 0.4598775021184915, -0.1350110200102546,
    -0.08544127388202662, 0.035226291885709554,
    // db4
    0.23037781330889645, 0.7148465705529156, 0.630880767929859, -0.02798376941685959,
    -0.18703481171909309, 0.03084138183556063, 0.03288301166688517, -0.010597401785069018,
    // db5
    0.16010239797419293, 0.6038292697971896, 0.724308528437773, 0.13842814590132088,
    -0.242294887066382, -0.03224486958463847, 0.0775714938400457, -0.006241490212798271,
    -0.012580751999081994, 0.003335725285473771,
    // db6
    0.1115407433501094, 0.4946238903984529, 0.7511339080210949, 0.315250351709198,
    -0.2262646939654393, -0.12976686756726188, 0.09750160558732306, 0.027522865530305606,
    -0.03158203931748598, 0.0005538422011615001, 0.0047772575109455056, -0.0010773010853084794,
    // db7
    0.07785205408500923, 0.3965393194819175, 0.7291320908462354, 0.46978228740519296,
    -0.14390600392856523, -0.22403618499387515, 0.07130921926683047, 0.08061260915108304,
    -0.03802993693501441, -0.016574541630666902, 0.012550998556099856, 0.00042957797292136684,
    -0.0018016407040474935, 0.0003537137999745206,
    // db8
    0.05441584224310395, 0.3128715909142996, 0.6756307362972892, 0.5853546836542065,
    -0.015829105256348515, -0.2840155429615464, 0.00047248457391308016, 0.12874742662047872,
    -0.01736930100180785, -0.04408825393079459, 0.013981027917398262, 0.008746094047405749,
    -0.004870352993451561, -0.0003917403733769474, 0.0006754494064505685, -0.00011747678412476935,
    // db9
    0.03807794736387834, 0.24383467461259023, 0.6048231236901112, 0.6572880780513,
    0.13319738582500756, -0.2932737832791743, -0.096840783222976, 0.14854074933810588,
    0.03072568147933388, -0.06763282906133072, 0.000250947114831909, 0.02236166212367897,
    -0.004723204757751389, -0.004281503682463433, 0.0018476468830562285, 0.00023038576352319616,
    -0.00025196318894271045, 3.9347320316271636e-05,
    // db10
    0.02667005790055555, 0.18817680007769153, 0.5272011889317257, 0.6884590394536034,
    0.28117234366057847, -0.24984642432731513, -0.19594627437737813, 0.12736934033579547,
    0.09305736460356871, -0.07139414716639458, -0.02945753682187686, 0.03321267405934137,
    0.0036065535669560058, -0.01073317548333054, 0.0013953517470529002, 0.0019924052951850566,
    -0.0006858566949597118, -0.00011646685512928554, 9.35886703200696e-05, -1.3264202894521243e-05,
};

// "haar" / "db<p>", 1 <= p <= 10 -> p; 0: no such wavelet
int wavelet_order(const char *name) {
  if (!std::strcmp(name, "haar")) return 1;
  if (name[0] != 'd' || name[1] != 'b' || name[2] < '1' || name[2] > '9') return 0;
  int p = name[2] - '0';
  if (name[3] == '0' && p == 1 && !name[4]) return 10;
  return name[3] ? 0 : p;
}

int wavelet_lookup(const char *name, const double **h, long long *ntaps) {
  if (!name) return fail(PDSP_ERR_BAD_ARG, "wavelet name is null");
  const int p = wavelet_order(name);
  if (p < 1 || p > kDaubechiesMax)
    return fail(PDSP_ERR_BAD_ARG, "unknown wavelet \"%.32s\" (haar, db1 ... db10)", name);
  *h = kDaubechies + (long long)p * (p - 1);  // 2 + 4 + ... + 2 (p - 1) taps come first
  *ntaps = 2 * p;
  return PDSP_OK;
}

int check_dwt_taps(const double *h, long long ntaps) {
  if (ntaps < 2 || ntaps > kDwtMaxTaps || ntaps % 2)
    return fail(PDSP_ERR_BAD_ARG, "the scaling filter must have an even number of taps, 2 ... %lld, got %lld", kDwtMaxTaps,
                ntaps);
  if (!h) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  for (long long m = 0; m < ntaps / 2; ++m) {
    double s = 0.0;
    for (long long k = 0; k + 2 * m < ntaps; ++k) s += h[k] * h[k + 2 * m];
    if (!(std::fabs(s - (m == 0 ? 1.0 : 0.0)) <= 1e-10))
      return fail(PDSP_ERR_BAD_ARG, "the taps are not an orthonormal scaling filter: sum_k h[k] h[k + %lld] is not %d "
                  "within 1e-10", 2 * m, m == 0 ? 1 : 0);
  }
  return PDSP_OK;
}

int check_dwt_levels(int levels) {
  if (levels < 1) return fail(PDSP_ERR_BAD_ARG, "levels must be >= 1, got %d", levels);
  return PDSP_OK;
}

int check_dwt_len(long long len, int levels) {
  if (levels > 62 || len < 1 || len % (1LL << levels))
    return fail(PDSP_ERR_BAD_ARG, "len must be a positive multiple of 2^levels (levels = %d), got %lld", levels, len);
  return PDSP_OK;
}

template <typename T>
int dwt_t(const pdsp_dwt *cw, bool inverse, long long batch, const T *in, long long len, long long in_stride, T *out,
          long long out_stride, hipStream_t s) {
  if (!cw) return fail(PDSP_ERR_BAD_ARG, "dwt is null");
  pdsp_dwt *const w = const_cast<pdsp_dwt *>(cw);
  const long long f = (long long)w->hg.size() / 2;
  if (batch < 0) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 0, got %lld", batch);
  if (int rc = check_dwt_len(len, w->levels)) return rc;
  if (in_stride < len || out_stride < len)
    return fail(PDSP_ERR_BAD_ARG, "strides must be >= len = %lld, got %lld (input) and %lld (output)", len, in_stride,
                out_stride);
  long long ic = 0, oc = 0;
  if (int rc = row_extents(batch, {{in_stride, len, &ic}, {out_stride, len, &oc}})) return rc;
  if (batch == 0) return PDSP_OK;
  if (!in || !out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  DwtTile t;
  if (int rc = dwt_tile_checked(f, w->levels, len, sizeof(T), inverse, &t)) return rc;
  long long blocks = 0;
  if (__builtin_mul_overflow(batch, t.tiles, &blocks) || blocks > 0x7fffffffLL)
    return fail(PDSP_ERR_BAD_ARG, "batch too large: %lld rows of %lld tiles", batch, t.tiles);
  // resident: a workgroup loads its whole row before it stores anything, so the exact in-place call is safe.  Any other
  // overlap lets one workgroup's stores reach another's loads: byte ranges of the whole strided extents
  const bool in_place = t.resident && exact_in_place(out, out_stride, in, in_stride);
  if (!in_place && host_ranges_overlap(in, (size_t)ic * sizeof(T), out, (size_t)oc * sizeof(T)))
    return fail(PDSP_ERR_BAD_ARG, t.resident ? "output overlaps input (only out == in with equal strides may share bytes)"
                                             : "output overlaps input (rows beyond the resident path share no bytes)");
  if (int rc = require_device()) return rc;
  T *&hg = w->slot<T>();
  if (int rc = first_use_table(*w, hg, s, "tap table", [&] { return std::vector<T>(w->hg.begin(), w->hg.end()); }))
    return rc;
  DeviceGuard dg(w->device);
  PDSP_HIP_TRY(dg.err);
  return dwt_dev<T>(t, hg, (int)f, w->levels, inverse, batch, in, len, in_stride, out, out_stride, s);
}

// The host forms ride the packed features' scaffold on the cached plan of 64 points (its stream, its lock, its
// device); the transform's own object lives for the call.  Buffer: out | in.
int dwt_host(bool inverse, const double *in, long long batch, long long len, const char *name, const double *taps,
             long long ntaps, int levels, double *out) {
  pdsp_dwt *w = nullptr;
  if (int rc = pdsp_dwt_create(-1, name, taps, ntaps, levels, &w)) return rc;
  const HandleOwner<pdsp_dwt> own(w);
  if (batch < 0) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 0, got %lld", batch);
  if (int rc = check_dwt_len(len, levels)) return rc;
  long long count = 0;
  if (!host_count_ok(batch, len, &count)) return fail(PDSP_ERR_BAD_ARG, "batch %lld x length overflows", batch);
  if (batch == 0) return PDSP_OK;
  if (!in || !out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  DwtTile t;
  if (int rc = dwt_tile_checked((long long)w->hg.size() / 2, levels, len, sizeof(double), inverse, &t)) return rc;
  const size_t nx = (size_t)count;
  return packed_host_call(
      64, PDSP_WIN_RECT, 2 * nx,
      [&](pdsp_plan *, hipStream_t s, const double *, double *d) -> int {
        PDSP_HIP_TRY(hipMemcpyAsync(d + nx, in, nx * sizeof(double), hipMemcpyHostToDevice, s));
        return dwt_t<double>(w, inverse, batch, d + nx, len, len, d, len, s);
      },
      [&](const double *d) -> int {
        PDSP_HIP_TRY(hipMemcpy(out, d, nx * sizeof(double), hipMemcpyDeviceToHost));
        return PDSP_OK;
      });
}

}  // namespace

int pdsp_wavelet_taps(const char *name, double *out, long long *ntaps) {
  if (!ntaps) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const double *h = nullptr;
  if (int rc = wavelet_lookup(name, &h, ntaps)) return rc;
  if (out) std::memcpy(out, h, (size_t)*ntaps * sizeof(double));
  return PDSP_OK;
}

int pdsp_dwt_create(int device, const char *name_or_null, const double *taps_or_null, long long ntaps, int levels,
                    pdsp_dwt **out) {
  if (!out) return fail(PDSP_ERR_BAD_ARG, "out is null");
  *out = nullptr;
  if (int rc = check_dwt_levels(levels)) return rc;
  const double *h = taps_or_null;
  if (name_or_null) {
    if (taps_or_null) return fail(PDSP_ERR_BAD_ARG, "pass a wavelet name or taps, not both");
    if (int rc = wavelet_lookup(name_or_null, &h, &ntaps)) return rc;
  }
  if (int rc = check_dwt_taps(h, ntaps)) return rc;
  pdsp_dwt *w = new (std::nothrow) pdsp_dwt();
  if (!w) return fail(PDSP_ERR_BAD_ARG, "out of host memory");
  w->device = device < 0 ? -1 : device;
  w->levels = levels;
  w->hg.assign(h, h + ntaps);
  for (long long j = 0; j < ntaps; ++j) w->hg.push_back((j % 2 ? -1.0 : 1.0) * h[ntaps - 1 - j]);
  *out = w;
  return PDSP_OK;
}

int pdsp_dwt_destroy(pdsp_dwt *w) { return destroy_handle(w); }

long long pdsp_dwt_ntaps(const pdsp_dwt *w) { return w ? (long long)w->hg.size() / 2 : 0; }
int pdsp_dwt_levels(const pdsp_dwt *w) { return w ? w->levels : 0; }
int pdsp_dwt_taps(const pdsp_dwt *w, double *taps) {
  if (!w || !taps) return fail(PDSP_ERR_BAD_ARG, w ? "null buffer" : "dwt is null");
  std::memcpy(taps, w->hg.data(), w->hg.size() / 2 * sizeof(double));
  return PDSP_OK;
}

// The rule's own answer, whatever pdsp_set_dwt_tile says: every depth on a row the resident path holds (forward:
// len + len / 2 values within 160 KiB), the tiled path's limit beyond
int pdsp_dwt_max_levels(long long ntaps, long long len, int elem_bytes) {
  if (ntaps < 2 || ntaps > kDwtMaxTaps || ntaps % 2 || len < 1 || (elem_bytes != 4 && elem_bytes != 8)) return 0;
  int most = 0;
  while (most < 62 && len % (1LL << (most + 1)) == 0) ++most;
  if (len <= (1LL << 40) && (len + len / 2) * elem_bytes <= 163840) return most;
  const int tiled = dwt_tiled_max_levels(ntaps, (size_t)elem_bytes);
  return most < tiled ? most : tiled;
}

int pdsp_dwt_forward_f32(const pdsp_dwt *w, long long batch, const float *x, long long len, long long x_stride, float *y,
                         long long y_stride, pdsp_stream stream) {
  return dwt_t<float>(w, false, batch, x, len, x_stride, y, y_stride, (hipStream_t)stream);
}
int pdsp_dwt_forward_f64(const pdsp_dwt *w, long long batch, const double *x, long long len, long long x_stride,
                         double *y, long long y_stride, pdsp_stream stream) {
  return dwt_t<double>(w, false, batch, x, len, x_stride, y, y_stride, (hipStream_t)stream);
}
int pdsp_dwt_inverse_f32(const pdsp_dwt *w, long long batch, const float *c, long long len, long long c_stride, float *x,
                         long long x_stride, pdsp_stream stream) {
  return dwt_t<float>(w, true, batch, c, len, c_stride, x, x_stride, (hipStream_t)stream);
}
int pdsp_dwt_inverse_f64(const pdsp_dwt *w, long long batch, const double *c, long long len, long long c_stride,
                         double *x, long long x_stride, pdsp_stream stream) {
  return dwt_t<double>(w, true, batch, c, len, c_stride, x, x_stride, (hipStream_t)stream);
}

int pdsp_dwt_forward_host_f64(const double *x, long long batch, long long len, const char *name_or_null,
                              const double *taps_or_null, long long ntaps, int levels, double *y) {
  return dwt_host(false, x, batch, len, name_or_null, taps_or_null, ntaps, levels, y);
}
int pdsp_dwt_inverse_host_f64(const double *c, long long batch, long long len, const char *name_or_null,
                              const double *taps_or_null, long long ntaps, int levels, double *x) {
  return dwt_host(true, c, batch, len, name_or_null, taps_or_null, ntaps, levels, x);
}

int pdsp_set_dwt_tile(int mode) {
  const int prev = g_dwt_tile;
  if (mode >= 0 && (mode & 3) <= 2) g_dwt_tile = mode;
  return prev;
}

int pdsp_dev_dwt_tile(long long ntaps, int levels, long long len, int elem_bytes, int inverse, long long info[5]) {
  if (!info) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (ntaps < 2 || ntaps > kDwtMaxTaps || ntaps % 2)
    return fail(PDSP_ERR_BAD_ARG, "the scaling filter must have an even number of taps, 2 ... %lld, got %lld", kDwtMaxTaps,
                ntaps);
  if (int rc = check_dwt_levels(levels)) return rc;
  if (int rc = check_dwt_len(len, levels)) return rc;
  if (elem_bytes != 4 && elem_bytes != 8) return fail(PDSP_ERR_BAD_ARG, "elem_bytes must be 4 or 8, got %d", elem_bytes);
  DwtTile t;
  if (int rc = dwt_tile_checked(ntaps, levels, len, (size_t)elem_bytes, inverse != 0, &t)) return rc;
  const long long v[5] = {t.resident, t.tile, t.halo, (long long)t.lds_bytes, t.tiles};
  std::memcpy(info, v, sizeof(v));
  return PDSP_OK;
}

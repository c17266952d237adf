// pdsp_capi_resample.hip -- polyphase rate change (upfirdn / resample_poly): the resampler handle, the filter design, entry points, host forms.
// Host side only; calls upfirdn_dev and upfirdn_tile_checked (pdsp_kernels_resample.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "pdsp_host.h"

using namespace pdsp_host;

/* ---- polyphase rate change: upfirdn / resample_poly -------------------------- */

// A resampler is its tap table: no FFT size, so no plan.  The table is kept in f64, phase-major
// (g[p][j] = h[p + j up], up rows of T = ceil(ntaps / up), zero-padded), rounded once per precision and uploaded on
// first use (TableHandle, first_use_table).
struct pdsp_resampler : TableHandle {
  long long up = 1, down = 1, ntaps = 1, t0 = 0;
  std::vector<double> taps;  // as convolved (resample_poly: times up)
  std::vector<double> g;
  float *g32 = nullptr;
  double *g64 = nullptr;
  template <typename T>
  auto &slot() {
    if constexpr (sizeof(T) == 4) return g32;
    else return g64;
  }
};

namespace {

constexpr long long kResampleMaxRatio = 8192, kResampleMaxTaps = 8192;

long long gcd_ll(long long a, long long b) {
  while (b) {
    const long long t = a % b;
    a = b, b = t;
  }
  return a;
}

int check_resample_ratio(long long up, long long down) {
  if (up < 1 || down < 1) return fail(PDSP_ERR_BAD_ARG, "up and down must be >= 1, got up %lld, down %lld", up, down);
  if (up > kResampleMaxRatio || down > kResampleMaxRatio)
    return fail(PDSP_ERR_UNSUPPORTED_SIZE, "up and down must be <= %lld, got up %lld, down %lld", kResampleMaxRatio, up,
                down);
  return PDSP_OK;
}

int check_resample_ntaps(long long ntaps) {
  if (ntaps < 1) return fail(PDSP_ERR_BAD_ARG, "filter must have at least one tap, got %lld", ntaps);
  if (ntaps > kResampleMaxTaps)
    return fail(PDSP_ERR_UNSUPPORTED_SIZE, "filter of %lld taps exceeds the %lld a resampler holds", ntaps,
                kResampleMaxTaps);
  return PDSP_OK;
}

// I0(x), the power series sum_k ((x/2)^k / k!)^2, until a term falls below 1e-17 of the sum
double bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-17 * sum) break;
  }
  return sum;
}

// scipy.signal.firwin(2 half + 1, 1 / m, window=("kaiser", 5.0)) * up, half = 10 m, m = max(up, down): a sinc of
// cutoff 1 / m (Nyquist = 1) under a Kaiser window, normalised to unit gain at DC.  up, down already reduced.
void design_taps(long long up, long long down, std::vector<double> *h) {
  const long long m = up > down ? up : down, half = 10 * m, n = 2 * half + 1;
  const double c = 1.0 / (double)m, beta = 5.0, i0b = bessel_i0(beta);
  h->assign((size_t)n, 0.0);
  double sum = 0.0;
  for (long long i = 0; i < n; ++i) {
    const double t = (double)(i - half);
    const double a = M_PI * c * t;
    const double sinc = t == 0.0 ? 1.0 : std::sin(a) / a;
    const double r = t / (double)half;
    const double w = bessel_i0(beta * std::sqrt(1.0 - r * r)) / i0b;
    (*h)[(size_t)i] = c * sinc * w;
    sum += (*h)[(size_t)i];
  }
  for (double &v : *h) v = v / sum * (double)up;
}

int resampler_new(int device, long long up, long long down, std::vector<double> taps, long long t0,
                  pdsp_resampler **out) {
  pdsp_resampler *rs = new (std::nothrow) pdsp_resampler();
  if (!rs) return fail(PDSP_ERR_BAD_ARG, "out of host memory");
  rs->device = device < 0 ? -1 : device;
  rs->up = up, rs->down = down, rs->ntaps = (long long)taps.size(), rs->t0 = t0;
  const long long tn = (rs->ntaps + up - 1) / up;
  rs->g.assign((size_t)(up * tn), 0.0);
  for (long long i = 0; i < rs->ntaps; ++i) rs->g[(size_t)((i % up) * tn + i / up)] = taps[(size_t)i];
  rs->taps = std::move(taps);
  *out = rs;
  return PDSP_OK;
}

// The reduction scipy.signal.resample_poly makes: up, down by their gcd; equal -> the identity (one tap, 1);
// otherwise the given taps, or the default design, times up, and t0 = (ntaps - 1) / 2.
int resample_poly_setup(long long up, long long down, const double *taps, long long ntaps, long long *up_r,
                        long long *down_r, std::vector<double> *h, long long *t0) {
  if (int rc = check_resample_ratio(up, down)) return rc;
  if (taps)
    if (int rc = check_resample_ntaps(ntaps)) return rc;
  const long long gcd = gcd_ll(up, down);
  up /= gcd, down /= gcd;
  *up_r = up, *down_r = down;
  if (up == down) {
    h->assign(1, 1.0);
  } else if (taps) {
    h->assign(taps, taps + ntaps);
    for (double &v : *h) v *= (double)up;
  } else {
    const long long n = 20 * (up > down ? up : down) + 1;
    if (n > kResampleMaxTaps)
      return fail(PDSP_ERR_UNSUPPORTED_SIZE,
                  "the default filter for %lld/%lld has %lld taps, beyond the %lld a resampler holds (pass shorter taps)",
                  up, down, n, kResampleMaxTaps);
    design_taps(up, down, h);
  }
  *t0 = ((long long)h->size() - 1) / 2;
  return PDSP_OK;
}

int resample_len(const pdsp_resampler *rs, long long len, int full, long long *y_len) {
  if (len < 1) return fail(PDSP_ERR_BAD_ARG, "len must be >= 1, got %lld", len);
  long long v = 0;
  if (full ? !mad_ok(len - 1, rs->up, rs->ntaps - 1, &v) : !mad_ok(len, rs->up, rs->down - 1, &v))
    return fail(PDSP_ERR_BAD_ARG, "len %lld x up %lld overflows", len, rs->up);
  *y_len = full ? v / rs->down + 1 : v / rs->down;
  return PDSP_OK;
}

template <typename T>
int upfirdn_t(const pdsp_resampler *crs, long long batch, const T *x, long long len, long long x_stride, T *y,
              long long y_len, long long y_stride, hipStream_t s) {
  if (!crs) return fail(PDSP_ERR_BAD_ARG, "resampler is null");
  pdsp_resampler *const rs = const_cast<pdsp_resampler *>(crs);
  if (batch < 0 || y_len < 0) return fail(PDSP_ERR_BAD_ARG, "negative size (batch %lld, y_len %lld)", batch, y_len);
  if (len < 1) return fail(PDSP_ERR_BAD_ARG, "len must be >= 1, got %lld", len);
  if (x_stride < len || y_stride < y_len)
    return fail(PDSP_ERR_BAD_ARG, "strides must be >= len = %lld (x) and >= y_len = %lld (y), got x_stride %lld, y_stride %lld",
                len, y_len, x_stride, y_stride);
  long long xc = 0, yc = 0, q = 0;
  if (int rc = row_extents(batch, {{x_stride, len, &xc}, {y_stride, y_len, &yc}})) return rc;
  if (!mad_ok(y_len, rs->down, rs->t0 + rs->up * rs->down, &q))
    return fail(PDSP_ERR_BAD_ARG, "y_len %lld x down %lld overflows", y_len, rs->down);
  if (batch == 0 || y_len == 0) return PDSP_OK;
  if (!x || !y) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  // a tile reads samples that other tiles' outputs would overwrite: byte ranges of the whole strided extents
  if (host_ranges_overlap(x, (size_t)xc * sizeof(T), y, (size_t)yc * sizeof(T)))
    return fail(PDSP_ERR_BAD_ARG, "output overlaps input");
  if (int rc = require_device()) return rc;
  T *&g = rs->slot<T>();
  if (int rc = first_use_table(*rs, g, s, "tap table", [&] { return std::vector<T>(rs->g.begin(), rs->g.end()); }))
    return rc;
  DeviceGuard dg(rs->device);
  PDSP_HIP_TRY(dg.err);
  return upfirdn_dev<T>(g, rs->up, rs->down, rs->ntaps, rs->t0, batch, x, len, x_stride, y, y_len, y_stride, s);
}

// The host forms: one resampler, one device buffer x | y, the f64 kernel on the null stream (pdsp_fir_filter_host_f64's
// shape: f64 arithmetic whatever pdsp_set_host_precision says).
int resample_host(pdsp_resampler *rs, const double *x, long long batch, long long len, int full, double *y) {
  const HandleOwner<pdsp_resampler> own(rs);
  if (batch < 0) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 0, got %lld", batch);
  long long y_len = 0, xs = 0, ys = 0;
  if (int rc = resample_len(rs, len, full, &y_len)) return rc;
  if (!host_count_ok(batch, len, &xs) || !host_count_ok(batch, y_len, &ys))
    return fail(PDSP_ERR_BAD_ARG, "batch %lld x length overflows", batch);
  if (batch == 0) return PDSP_OK;
  if (!x || !y) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (int rc = require_device()) return rc;
  DeviceBuf sc;
  const size_t nx = (size_t)xs, ny = (size_t)ys;
  PDSP_HIP_TRY(hipMalloc((void **)&sc.d, (nx + ny) * sizeof(double)));
  PDSP_HIP_TRY(hipMemcpy(sc.d, x, nx * sizeof(double), hipMemcpyHostToDevice));
  if (int rc = upfirdn_t<double>(rs, batch, sc.d, len, len, sc.d + nx, y_len, y_len, nullptr)) return rc;
  PDSP_HIP_TRY(hipMemcpy(y, sc.d + nx, ny * sizeof(double), hipMemcpyDeviceToHost));
  return PDSP_OK;
}

}  // namespace

int pdsp_resampler_create(int device, long long up, long long down, const double *taps, long long ntaps, long long t0,
                          pdsp_resampler **out) {
  if (!out) return fail(PDSP_ERR_BAD_ARG, "out is null");
  *out = nullptr;
  if (int rc = check_resample_ratio(up, down)) return rc;
  if (int rc = check_resample_ntaps(ntaps)) return rc;
  if (!taps) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (t0 < 0 || t0 >= ntaps + up)
    return fail(PDSP_ERR_BAD_ARG, "t0 must be 0 ... ntaps + up - 1 = %lld, got %lld", ntaps + up - 1, t0);
  return resampler_new(device, up, down, std::vector<double>(taps, taps + ntaps), t0, out);
}

int pdsp_resampler_create_poly(int device, long long up, long long down, const double *taps_or_null, long long ntaps,
                               pdsp_resampler **out) {
  if (!out) return fail(PDSP_ERR_BAD_ARG, "out is null");
  *out = nullptr;
  std::vector<double> h;
  long long t0 = 0;
  if (int rc = resample_poly_setup(up, down, taps_or_null, ntaps, &up, &down, &h, &t0)) return rc;
  return resampler_new(device, up, down, std::move(h), t0, out);
}

int pdsp_resampler_destroy(pdsp_resampler *rs) { return destroy_handle(rs); }

long long pdsp_resampler_up(const pdsp_resampler *rs) { return rs ? rs->up : 0; }
long long pdsp_resampler_down(const pdsp_resampler *rs) { return rs ? rs->down : 0; }
long long pdsp_resampler_ntaps(const pdsp_resampler *rs) { return rs ? rs->ntaps : 0; }
long long pdsp_resampler_t0(const pdsp_resampler *rs) { return rs ? rs->t0 : 0; }
int pdsp_resampler_taps(const pdsp_resampler *rs, double *taps) {
  if (!rs || !taps) return fail(PDSP_ERR_BAD_ARG, rs ? "null buffer" : "resampler is null");
  std::memcpy(taps, rs->taps.data(), rs->taps.size() * sizeof(double));
  return PDSP_OK;
}

int pdsp_resample_output_len(const pdsp_resampler *rs, long long len, int full, long long *y_len) {
  if (!rs) return fail(PDSP_ERR_BAD_ARG, "resampler is null");
  if (!y_len) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  return resample_len(rs, len, full, y_len);
}

int pdsp_upfirdn_f32(const pdsp_resampler *rs, long long batch, const float *x, long long len, long long x_stride,
                     float *y, long long y_len, long long y_stride, pdsp_stream stream) {
  return upfirdn_t<float>(rs, batch, x, len, x_stride, y, y_len, y_stride, (hipStream_t)stream);
}
int pdsp_upfirdn_f64(const pdsp_resampler *rs, long long batch, const double *x, long long len, long long x_stride,
                     double *y, long long y_len, long long y_stride, pdsp_stream stream) {
  return upfirdn_t<double>(rs, batch, x, len, x_stride, y, y_len, y_stride, (hipStream_t)stream);
}

int pdsp_set_upfirdn_tile(int mode) {
  const int prev = g_upfirdn_tile;
  if (mode >= 0 && (mode & 15) <= 4) g_upfirdn_tile = mode;
  return prev;
}

int pdsp_dev_upfirdn_tile(long long up, long long down, long long ntaps, long long y_len, int elem_bytes,
                          long long info[9]) {
  if (!info) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (int rc = check_resample_ratio(up, down)) return rc;
  if (int rc = check_resample_ntaps(ntaps)) return rc;
  if (y_len < 1) return fail(PDSP_ERR_BAD_ARG, "y_len must be >= 1, got %lld", y_len);
  if (elem_bytes != 4 && elem_bytes != 8) return fail(PDSP_ERR_BAD_ARG, "elem_bytes must be 4 or 8, got %d", elem_bytes);
  UpfirdnTile t;
  if (int rc = upfirdn_tile_checked(up, down, ntaps, y_len, (size_t)elem_bytes, &t)) return rc;
  const long long v[9] = {t.r, t.win, t.gt, t.tn, t.tp, t.bper, t.span, (long long)t.lds_bytes, t.items};
  std::memcpy(info, v, sizeof(v));
  return PDSP_OK;
}

int pdsp_resample_design_f64(long long up, long long down, double *taps, long long *ntaps) {
  if (!ntaps) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  std::vector<double> h;
  long long t0 = 0;
  if (int rc = resample_poly_setup(up, down, nullptr, 0, &up, &down, &h, &t0)) return rc;
  *ntaps = (long long)h.size();
  if (taps) std::memcpy(taps, h.data(), h.size() * sizeof(double));
  return PDSP_OK;
}

int pdsp_resample_poly_host_f64(const double *x, long long batch, long long len, long long up, long long down,
                                const double *taps_or_null, long long ntaps, double *y) {
  pdsp_resampler *rs = nullptr;
  if (int rc = pdsp_resampler_create_poly(-1, up, down, taps_or_null, ntaps, &rs)) return rc;
  return resample_host(rs, x, batch, len, 0, y);
}

int pdsp_upfirdn_host_f64(const double *h, long long ntaps, const double *x, long long batch, long long len,
                          long long up, long long down, double *y) {
  pdsp_resampler *rs = nullptr;
  if (int rc = pdsp_resampler_create(-1, up, down, h, ntaps, 0, &rs)) return rc;
  return resample_host(rs, x, batch, len, 1, y);
}

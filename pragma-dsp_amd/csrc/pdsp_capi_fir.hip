// pdsp_capi_fir.hip -- FIR filtering (fused overlap-save) and the filter spectrum: validators, entry points, host form.
// Host side only; calls fir_filter_dev and fir_spectrum_dev (pdsp_kernels_fir.hip).
#include <hip/hip_runtime.h>

#include <vector>

#include "pdsp_host.h"

using namespace pdsp_host;

/* ---- FIR filtering: fused overlap-save --------------------------------------- */

namespace {

// Filters have at most N/2 taps (the tap count is checked ahead of the plan's size, behind its null check).
template <typename T>
int check_fir_plan(const pdsp_plan *plan, long long ntaps) {
  if (plan && ntaps < 1) return fail(PDSP_ERR_BAD_ARG, "filter must have at least one tap, got %lld", ntaps);
  if (int rc = check_packed_plan<T>(plan, "FIR filtering", false)) return rc;
  if (ntaps > plan->n / 2)
    return fail(PDSP_ERR_UNSUPPORTED_SIZE, "filter of %lld taps exceeds N/2 = %lld of the plan (no partitioned convolution)",
                ntaps, plan->n / 2);
  return PDSP_OK;
}

template <typename T>
int fir_spectrum_t(const pdsp_plan *plan, const T *taps, long long ntaps, T *h_re, T *h_im, hipStream_t s) {
  if (int rc = check_fir_plan<T>(plan, ntaps)) return rc;
  if (!taps || !h_re || !h_im) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  DeviceGuard g(plan->device);
  PDSP_HIP_TRY(g.err);
  return fir_spectrum_dev<T>(plan, taps, (int)ntaps, h_re, h_im, s);
}

template <typename T>
int fir_filter_t(const pdsp_plan *plan, long long batch, const T *x, long long len, long long x_stride, const T *h_re,
                 const T *h_im, long long ntaps, long long y_off, long long y_len, T *y, long long y_stride,
                 hipStream_t s) {
  if (int rc = check_fir_plan<T>(plan, ntaps)) return rc;
  if (batch < 0 || len < 0 || y_off < 0 || y_len < 0)
    return fail(PDSP_ERR_BAD_ARG, "negative size (batch %lld, len %lld, y_off %lld, y_len %lld)", batch, len, y_off, y_len);
  if (x_stride < 0 || y_stride < 0) return fail(PDSP_ERR_BAD_ARG, "negative stride");
  long long full = 0, xc = 0, yc = 0;
  if (__builtin_add_overflow(len, ntaps - 1, &full) || y_off > full || y_len > full - y_off)
    return fail(PDSP_ERR_BAD_ARG, "outputs [%lld, %lld + %lld) beyond the full convolution of %lld samples", y_off, y_off,
                y_len, full);
  if (batch > 1 && y_stride < y_len) return fail(PDSP_ERR_BAD_ARG, "y_stride %lld < y_len %lld", y_stride, y_len);
  if (int rc = row_extents(batch, {{x_stride, len, &xc}, {y_stride, y_len, &yc}})) return rc;
  if (batch == 0 || y_len == 0) return PDSP_OK;
  if (!y || (len > 0 && (!x || !h_re || !h_im))) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  // blocks of a row read input that other blocks overwrite when y shares bytes with x: the result would depend on
  // the order in which workgroups run.  Byte ranges of the whole strided extent, as planes_overlap()
  if (len > 0 && host_ranges_overlap(x, (size_t)xc * sizeof(T), y, (size_t)yc * sizeof(T)))
    return fail(PDSP_ERR_BAD_ARG, "output overlaps input");
  // an even filter runs with one zero tap more (same H): P odd makes hop = N - P + 1 even, the aligned fast path
  const int p = (int)(ntaps % 2 == 1 ? ntaps : ntaps + 1);
  const long long hop = plan->n - (p - 1);
  const long long nblk = (y_len + hop - 1) / hop;
  long long items = 0;
  if (__builtin_mul_overflow(batch, nblk, &items) || items > 0x7fffffffLL)
    return fail(PDSP_ERR_BAD_ARG, "batch too large: %lld rows of %lld blocks", batch, nblk);
  DeviceGuard g(plan->device);
  PDSP_HIP_TRY(g.err);
  if (len == 0) {  // nothing but zero padding: y = 0
    PDSP_HIP_TRY(hipMemset2DAsync(y, (size_t)(batch > 1 ? y_stride : y_len) * sizeof(T), 0, (size_t)y_len * sizeof(T),
                                  (size_t)batch, s));
    return PDSP_OK;
  }
  return fir_filter_dev<T>(plan, batch, x, len, x_stride, h_re, h_im, p, y_off, y_len, y, y_stride, nblk, s);
}

// Block size of the host form (and of FirFilter's default): DESIGN.md, "FIR filtering".
long long fir_block_for(long long ntaps) {
  long long n = 4096;
  while (n < 8 * ntaps && n < 16384) n *= 2;
  while (n / 2 < ntaps) n *= 2;  // never below 2P (the caller has checked ntaps <= 8192)
  return n;
}

}  // namespace

int pdsp_fir_spectrum_f32(const pdsp_plan *plan, const float *taps, long long ntaps, float *h_re, float *h_im,
                          pdsp_stream stream) {
  return fir_spectrum_t<float>(plan, taps, ntaps, h_re, h_im, (hipStream_t)stream);
}
int pdsp_fir_spectrum_f64(const pdsp_plan *plan, const double *taps, long long ntaps, double *h_re, double *h_im,
                          pdsp_stream stream) {
  return fir_spectrum_t<double>(plan, taps, ntaps, h_re, h_im, (hipStream_t)stream);
}
int pdsp_fir_filter_f32(const pdsp_plan *plan, long long batch, const float *x, long long len, long long x_stride,
                        const float *h_re, const float *h_im, long long ntaps, long long y_off, long long y_len, float *y,
                        long long y_stride, pdsp_stream stream) {
  return fir_filter_t<float>(plan, batch, x, len, x_stride, h_re, h_im, ntaps, y_off, y_len, y, y_stride,
                             (hipStream_t)stream);
}
int pdsp_fir_filter_f64(const pdsp_plan *plan, long long batch, const double *x, long long len, long long x_stride,
                        const double *h_re, const double *h_im, long long ntaps, long long y_off, long long y_len,
                        double *y, long long y_stride, pdsp_stream stream) {
  return fir_filter_t<double>(plan, batch, x, len, x_stride, h_re, h_im, ntaps, y_off, y_len, y, y_stride,
                              (hipStream_t)stream);
}

long long pdsp_fir_block_size(long long ntaps) {
  if (ntaps < 1 || ntaps > 8192) return 0;
  return fir_block_for(ntaps);
}

int pdsp_fir_output_range(long long len, long long ntaps, int mode, long long *y_off, long long *y_len) {
  if (len < 1 || ntaps < 1) return fail(PDSP_ERR_BAD_ARG, "signal and filter must not be empty (len %lld, ntaps %lld)", len, ntaps);
  if (!y_off || !y_len) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const long long m = len < ntaps ? len : ntaps;
  switch (mode) {
    case PDSP_FIR_FULL: *y_off = 0, *y_len = len + ntaps - 1; break;
    case PDSP_FIR_SAME: *y_off = (m - 1) / 2, *y_len = len > ntaps ? len : ntaps; break;
    case PDSP_FIR_VALID: *y_off = m - 1, *y_len = (len > ntaps ? len - ntaps : ntaps - len) + 1; break;
    case PDSP_FIR_FILTER: *y_off = 0, *y_len = len; break;
    default: return fail(PDSP_ERR_BAD_ARG, "unknown FIR mode %d", mode);
  }
  return PDSP_OK;
}

int pdsp_fir_filter_host_f64(const double *x, long long batch, long long len, const double *taps, long long ntaps,
                             int mode, double *y) {
  if (batch < 0) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 0, got %lld", batch);
  if (ntaps < 1) return fail(PDSP_ERR_BAD_ARG, "filter must have at least one tap, got %lld", ntaps);
  long long y_off = 0, y_len = 0;
  if (int rc = pdsp_fir_output_range(len, ntaps, mode, &y_off, &y_len)) return rc;
  if (ntaps > 8192)
    return fail(PDSP_ERR_UNSUPPORTED_SIZE, "filter of %lld taps exceeds N/2 = 8192 of the largest block (no partitioned convolution)",
                ntaps);
  long long xs = 0, ys = 0;
  if (!host_count_ok(batch, len, &xs) || !host_count_ok(batch, y_len, &ys))
    return fail(PDSP_ERR_BAD_ARG, "batch %lld x length overflows", batch);
  if (batch == 0) return PDSP_OK;
  if (!x || !taps || !y) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (int rc = require_device()) return rc;
  CachedPlan cp;
  if (int rc = cached_plan(fir_block_for(ntaps), &cp)) return rc;
  const long long bins = cp.plan->n / 2 + 1;
  DeviceBuf sc;
  const size_t nx = (size_t)xs, ny = (size_t)ys, nh = (size_t)(2 * bins);
  PDSP_HIP_TRY(hipMalloc((void **)&sc.d, (nx + ny + nh + (size_t)ntaps) * sizeof(double)));
  double *dx = sc.d, *dy = sc.d + nx, *dh = sc.d + nx + ny, *dt = dh + nh;
  PDSP_HIP_TRY(hipMemcpy(dx, x, nx * sizeof(double), hipMemcpyHostToDevice));
  PDSP_HIP_TRY(hipMemcpy(dt, taps, (size_t)ntaps * sizeof(double), hipMemcpyHostToDevice));
  if (int rc = fir_spectrum_t<double>(cp.plan, dt, ntaps, dh, dh + bins, nullptr)) return rc;
  if (int rc = fir_filter_t<double>(cp.plan, batch, dx, len, len, dh, dh + bins, ntaps, y_off, y_len, dy, y_len, nullptr))
    return rc;
  PDSP_HIP_TRY(hipMemcpy(y, dy, ny * sizeof(double), hipMemcpyDeviceToHost));
  return PDSP_OK;
}

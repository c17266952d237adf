// pdsp_capi_dct.hip -- DCT-II and DCT-III: validators, entry points, host form.
// Host side only; calls dct_dev (pdsp_kernels_dct.hip).
#include <hip/hip_runtime.h>

#include <cmath>

#include "pdsp_host.h"

using namespace pdsp_host;

/* ---- discrete cosine transform, types 2 and 3 ------------------------------ */

namespace {

int check_dct_type_norm(int type, int norm) {
  if (type != 2 && type != 3) return fail(PDSP_ERR_BAD_ARG, "DCT type must be 2 or 3, got %d", type);
  if (norm < PDSP_DCT_BACKWARD || norm > PDSP_DCT_FORWARD)
    return fail(PDSP_ERR_BAD_ARG, "DCT norm must be 0 (backward), 1 (ortho) or 2 (forward), got %d", norm);
  return PDSP_OK;
}

// scipy's norm as the kernels' two scalars, computed in f64 and rounded once: g for every output (type 2) or input
// (type 3), g0 for index 0 instead
void dct_scales(long long n, int type, int norm, double *g, double *g0) {
  const double nn = (double)n;
  if (norm == PDSP_DCT_FORWARD) {
    *g = *g0 = 1.0 / (2.0 * nn);
  } else if (norm == PDSP_DCT_ORTHO) {
    *g = 1.0 / std::sqrt(2.0 * nn);
    *g0 = type == 2 ? 1.0 / std::sqrt(4.0 * nn) : 1.0 / std::sqrt(nn);
  } else {
    *g = *g0 = 1.0;
  }
}

template <typename T>
int dct_t(const pdsp_plan *plan, long long batch, const T *x, long long x_stride, int type, int norm, T *y,
          long long y_stride, hipStream_t s) {
  if (int rc = check_packed_plan<T>(plan, "DCT", true)) return rc;
  const long long n = plan->n;
  if (batch < 1) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 1, got %lld", batch);
  if (x_stride < n || y_stride < n)
    return fail(PDSP_ERR_BAD_ARG, "strides must be >= N = %lld, got x_stride %lld, y_stride %lld", n, x_stride, y_stride);
  if (int rc = check_dct_type_norm(type, norm)) return rc;
  long long xc = 0, yc = 0;
  if (int rc = row_extents(batch, {{x_stride, n, &xc}, {y_stride, n, &yc}})) return rc;
  if (batch > 0x7fffffffLL) return fail(PDSP_ERR_BAD_ARG, "batch too large: %lld", batch);
  if (!x || !y) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  // exact in place is safe (each row is loaded in full by its own workgroup before that workgroup's first barrier);
  // any other overlap would let one row's stores reach another row's loads
  if (!exact_in_place(y, y_stride, x, x_stride) && host_ranges_overlap(y, (size_t)yc * sizeof(T), x, (size_t)xc * sizeof(T)))
    return fail(PDSP_ERR_BAD_ARG, "output overlaps input (only y == x with y_stride == x_stride may share bytes)");
  double g = 1.0, g0 = 1.0;
  dct_scales(n, type, norm, &g, &g0);
  DeviceGuard dg(plan->device);
  PDSP_HIP_TRY(dg.err);
  return dct_dev<T>(plan, batch, x, x_stride, type, (T)g, (T)g0, y, y_stride, s);
}

}  // namespace

int pdsp_dct_f32(const pdsp_plan *plan, long long batch, const float *x, long long x_stride, int type, int norm,
                 float *y, long long y_stride, pdsp_stream stream) {
  return dct_t<float>(plan, batch, x, x_stride, type, norm, y, y_stride, (hipStream_t)stream);
}
int pdsp_dct_f64(const pdsp_plan *plan, long long batch, const double *x, long long x_stride, int type, int norm,
                 double *y, long long y_stride, pdsp_stream stream) {
  return dct_t<double>(plan, batch, x, x_stride, type, norm, y, y_stride, (hipStream_t)stream);
}

int pdsp_dct_host_f64(const double *x, long long batch, long long n, int type, int norm, double *y) {
  if (int rc = check_packed_size(n, "DCT")) return rc;
  if (batch < 1) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 1, got %lld", batch);
  if (int rc = check_dct_type_norm(type, norm)) return rc;
  long long count = 0;
  if (batch > 0x7fffffffLL || !host_count_ok(batch, n, &count))
    return fail(PDSP_ERR_BAD_ARG, "batch %lld x %lld overflows", batch, n);
  if (!x || !y) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const size_t nx = (size_t)count;
  return packed_host_call(
      n, PDSP_WIN_RECT, nx,
      [&](pdsp_plan *plan, hipStream_t s, const double *, double *d) -> int {
        PDSP_HIP_TRY(hipMemcpyAsync(d, x, nx * sizeof(double), hipMemcpyHostToDevice, s));
        return dct_t<double>(plan, batch, d, n, type, norm, d, n, s);  // in place
      },
      [&](const double *d) -> int {
        PDSP_HIP_TRY(hipMemcpy(y, d, nx * sizeof(double), hipMemcpyDeviceToHost));
        return PDSP_OK;
      });
}

// pdsp_capi_hilbert.hip -- Hilbert transform, analytic signal, envelope and phase: validators, entry points, host form.
// Host side only; calls hilbert_dev (pdsp_kernels_hilbert.hip).
#include <hip/hip_runtime.h>


#include "pdsp_host.h"

using namespace pdsp_host;

/* ---- Hilbert transform, analytic signal, envelope and phase ---------------- */

namespace {

int check_hilbert_mode(int out_mode) {
  if (out_mode < PDSP_HILBERT_ANALYTIC || out_mode > PDSP_HILBERT_PHASE)
    return fail(PDSP_ERR_BAD_ARG, "Hilbert output must be 0 (analytic), 1 (imag), 2 (envelope) or 3 (phase), got %d",
                out_mode);
  return PDSP_OK;
}

template <typename T>
int hilbert_t(const pdsp_plan *plan, long long batch, const T *x, long long x_stride, long long len, int out_mode, T *y,
              long long y_stride, hipStream_t s) {
  if (int rc = check_packed_plan<T>(plan, "the Hilbert transform", false)) return rc;
  const long long n = plan->n;
  if (batch < 1) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 1, got %lld", batch);
  if (len < 1 || len > n) return fail(PDSP_ERR_BAD_ARG, "len must be 1 ... N = %lld, got %lld", n, len);
  if (int rc = check_hilbert_mode(out_mode)) return rc;
  const long long yn = out_mode == PDSP_HILBERT_ANALYTIC ? 2 * n : n;  // values per output row
  if (x_stride < len || y_stride < yn)
    return fail(PDSP_ERR_BAD_ARG, "strides must be >= len = %lld (x) and >= %lld (y), got x_stride %lld, y_stride %lld",
                len, yn, x_stride, y_stride);
  long long xc = 0, yc = 0;
  if (int rc = row_extents(batch, {{x_stride, len, &xc}, {y_stride, yn, &yc}})) return rc;
  if (batch > 0x7fffffffLL) return fail(PDSP_ERR_BAD_ARG, "batch too large: %lld", batch);
  if (!x || !y) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  // exact in place is safe in the N-out modes (a row is loaded in full by its own workgroup before that workgroup's
  // first barrier, and a thread stores only to the samples it has just re-read); any other overlap would let one
  // row's stores reach another row's loads, and ANALYTIC writes two values per sample
  const bool in_place = out_mode != PDSP_HILBERT_ANALYTIC && exact_in_place(y, y_stride, x, x_stride);
  if (!in_place && host_ranges_overlap(y, (size_t)yc * sizeof(T), x, (size_t)xc * sizeof(T)))
    return fail(PDSP_ERR_BAD_ARG, "output overlaps input (only y == x with y_stride == x_stride may share bytes, and "
                                  "not in analytic mode)");
  DeviceGuard dg(plan->device);
  PDSP_HIP_TRY(dg.err);
  return hilbert_dev<T>(plan, batch, x, x_stride, len, out_mode, y, y_stride, s);
}

}  // namespace

int pdsp_hilbert_f32(const pdsp_plan *plan, long long batch, const float *x, long long x_stride, long long len,
                     int out_mode, float *y, long long y_stride, pdsp_stream stream) {
  return hilbert_t<float>(plan, batch, x, x_stride, len, out_mode, y, y_stride, (hipStream_t)stream);
}
int pdsp_hilbert_f64(const pdsp_plan *plan, long long batch, const double *x, long long x_stride, long long len,
                     int out_mode, double *y, long long y_stride, pdsp_stream stream) {
  return hilbert_t<double>(plan, batch, x, x_stride, len, out_mode, y, y_stride, (hipStream_t)stream);
}

int pdsp_hilbert_host_f64(const double *x, long long batch, long long len, long long n, int out_mode, double *y) {
  if (int rc = check_packed_size(n, "the Hilbert transform")) return rc;
  if (batch < 1) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 1, got %lld", batch);
  if (len < 1 || len > n) return fail(PDSP_ERR_BAD_ARG, "len must be 1 ... N = %lld, got %lld", n, len);
  if (int rc = check_hilbert_mode(out_mode)) return rc;
  const long long yn = out_mode == PDSP_HILBERT_ANALYTIC ? 2 * n : n;
  long long xcount = 0, ycount = 0;
  if (batch > 0x7fffffffLL || !host_count_ok(batch, len, &xcount) || !host_count_ok(batch, yn, &ycount))
    return fail(PDSP_ERR_BAD_ARG, "batch %lld x %lld overflows", batch, n);
  if (!x || !y) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  // buffer: y | x, rows of n values on the device whatever len is (the wide path's layout)
  const size_t ny = (size_t)ycount, nx = (size_t)(batch * n);
  return packed_host_call(
      n, PDSP_WIN_RECT, ny + nx,
      [&](pdsp_plan *plan, hipStream_t s, const double *, double *d) -> int {
        PDSP_HIP_TRY(hipMemcpy2DAsync(d + ny, (size_t)n * sizeof(double), x, (size_t)len * sizeof(double),
                                      (size_t)len * sizeof(double), (size_t)batch, hipMemcpyHostToDevice, s));
        return hilbert_t<double>(plan, batch, d + ny, n, len, out_mode, d, yn, s);
      },
      [&](const double *d) -> int {
        PDSP_HIP_TRY(hipMemcpy(y, d, ny * sizeof(double), hipMemcpyDeviceToHost));
        return PDSP_OK;
      });
}

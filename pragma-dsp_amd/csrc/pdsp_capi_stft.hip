// pdsp_capi_stft.hip -- the complex short-time transform and its overlap-add inverse: validators, entry points, host forms.
// Host side only; calls stft_complex_dev and istft_dev (pdsp_kernels_stft.hip).
#include <hip/hip_runtime.h>

#include <climits>
#include <utility>

#include "pdsp_host.h"

using namespace pdsp_host;

/* ---- short-time transform (complex bins) and its overlap-add inverse -------- */

namespace {

template <typename T>
int stft_complex_t(const pdsp_plan *plan, long long batch, const T *frames, long long frame_len, long long frame_stride,
                   const T *window, T *re_out, T *im_out, hipStream_t s) {
  if (int rc = check_packed_plan<T>(plan, "STFT", false)) return rc;
  if (batch < 1) return fail(PDSP_ERR_BAD_ARG, "frames must be >= 1, got %lld", batch);
  if (frame_len < 1) return fail(PDSP_ERR_BAD_ARG, "frame_len must be >= 1, got %lld", frame_len);
  if (frame_stride < 1) return fail(PDSP_ERR_BAD_ARG, "frame_stride (hop) must be >= 1, got %lld", frame_stride);
  if (batch > 0x7fffffffLL) return fail(PDSP_ERR_BAD_ARG, "batch too large: %lld", batch);
  const long long n = plan->n, bins = n / 2 + 1, used = frame_len < n ? frame_len : n;
  long long in_count = 0, out_count = 0;
  if (int rc = row_extents(batch, {{frame_stride, used, &in_count}, {bins, bins, &out_count}})) return rc;
  if (!frames || !re_out || !im_out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const size_t ib = (size_t)in_count * sizeof(T), ob = (size_t)out_count * sizeof(T), wb = (size_t)n * sizeof(T);
  if (host_ranges_overlap(re_out, ob, frames, ib) || host_ranges_overlap(im_out, ob, frames, ib) ||
      host_ranges_overlap(re_out, ob, im_out, ob) || host_ranges_overlap(re_out, ob, window, wb) ||
      host_ranges_overlap(im_out, ob, window, wb))
    return fail(PDSP_ERR_BAD_ARG, "output overlaps input");
  DeviceGuard g(plan->device);
  PDSP_HIP_TRY(g.err);
  return stft_complex_dev<T>(plan, batch, frames, used, frame_stride, window, re_out, im_out, s);
}

template <typename T>
int istft_t(const pdsp_plan *plan, long long frames, const T *re_in, const T *im_in, long long hop, const T *window, T *out,
            hipStream_t s) {
  if (int rc = check_packed_plan<T>(plan, "STFT", false)) return rc;
  if (frames < 1) return fail(PDSP_ERR_BAD_ARG, "frames must be >= 1, got %lld", frames);
  if (hop < 1) return fail(PDSP_ERR_BAD_ARG, "hop must be >= 1, got %lld", hop);
  if (frames > 0x7fffffffLL) return fail(PDSP_ERR_BAD_ARG, "batch too large: %lld", frames);
  const long long n = plan->n, bins = n / 2 + 1;
  long long total = 0, in_count = 0;
  if (!mad_ok(frames - 1, hop, n, &total) || !mad_ok(frames, bins, 0, &in_count) || total > (LLONG_MAX / 8) ||
      in_count > (LLONG_MAX / 8))
    return fail(PDSP_ERR_BAD_ARG, "frames %lld x hop %lld overflows", frames, hop);
  if (!re_in || !im_in || !out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const size_t ib = (size_t)in_count * sizeof(T), ob = (size_t)total * sizeof(T), wb = (size_t)n * sizeof(T);
  if (host_ranges_overlap(out, ob, re_in, ib) || host_ranges_overlap(out, ob, im_in, ib) ||
      host_ranges_overlap(out, ob, window, wb))
    return fail(PDSP_ERR_BAD_ARG, "output overlaps input");
  DeviceGuard g(plan->device);
  PDSP_HIP_TRY(g.err);
  return istft_dev<T>(plan, frames, re_in, im_in, hop, window, out, s);
}

// Host forms: size, range and window type in the order of the device forms; the plan and its window come from the
// host entry points' plan cache.
int stft_host_checks(long long fft_size, long long hop, int window_type) {
  if (int rc = check_packed_size(fft_size, "STFT")) return rc;
  if (hop < 1) return fail(PDSP_ERR_BAD_ARG, "hop must be >= 1, got %lld", hop);
  if (window_type < PDSP_WIN_RECT || window_type > PDSP_WIN_BLACKMAN)
    return fail(PDSP_ERR_WINDOW_TYPE, "Unsupported window type: %d", window_type);
  return PDSP_OK;
}

}  // namespace

int pdsp_stft_complex_f32(const pdsp_plan *plan, long long batch, const float *frames, long long frame_len,
                          long long frame_stride, const float *window, float *re_out, float *im_out, pdsp_stream stream) {
  return stft_complex_t<float>(plan, batch, frames, frame_len, frame_stride, window, re_out, im_out, (hipStream_t)stream);
}
int pdsp_stft_complex_f64(const pdsp_plan *plan, long long batch, const double *frames, long long frame_len,
                          long long frame_stride, const double *window, double *re_out, double *im_out,
                          pdsp_stream stream) {
  return stft_complex_t<double>(plan, batch, frames, frame_len, frame_stride, window, re_out, im_out, (hipStream_t)stream);
}
int pdsp_istft_f32(const pdsp_plan *plan, long long frames, const float *re_in, const float *im_in, long long hop,
                   const float *window, float *out, pdsp_stream stream) {
  return istft_t<float>(plan, frames, re_in, im_in, hop, window, out, (hipStream_t)stream);
}
int pdsp_istft_f64(const pdsp_plan *plan, long long frames, const double *re_in, const double *im_in, long long hop,
                   const double *window, double *out, pdsp_stream stream) {
  return istft_t<double>(plan, frames, re_in, im_in, hop, window, out, (hipStream_t)stream);
}

int pdsp_set_istft_chunk_frames(int frames) { return std::exchange(g_istft_chunk_frames, frames > 0 ? frames : 0); }

int pdsp_stft_host_f64(const double *signal, long long len, long long fft_size, long long hop, int window_type,
                       double *re_out, double *im_out) {
  if (int rc = stft_host_checks(fft_size, hop, window_type)) return rc;
  if (len < fft_size)
    return fail(PDSP_ERR_INPUT_LENGTH, "signal length %lld is shorter than one frame (%lld)", len, fft_size);
  const long long frames = 1 + (len - fft_size) / hop, bins = fft_size / 2 + 1;
  if (frames > 0x7fffffffLL || len > (1LL << 40)) return fail(PDSP_ERR_BAD_ARG, "signal too long: %lld samples", len);
  if (!signal || !re_out || !im_out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const size_t nx = (size_t)len, ny = (size_t)(frames * bins);  // buffer: signal | re | im
  return packed_host_call(
      fft_size, window_type, nx + 2 * ny,
      [&](pdsp_plan *plan, hipStream_t s, const double *win, double *d) -> int {
        PDSP_HIP_TRY(hipMemcpyAsync(d, signal, nx * sizeof(double), hipMemcpyHostToDevice, s));
        return stft_complex_t<double>(plan, frames, d, fft_size, hop, win, d + nx, d + nx + ny, s);
      },
      [&](const double *d) -> int {
        PDSP_HIP_TRY(hipMemcpy(re_out, d + nx, ny * sizeof(double), hipMemcpyDeviceToHost));
        PDSP_HIP_TRY(hipMemcpy(im_out, d + nx + ny, ny * sizeof(double), hipMemcpyDeviceToHost));
        return PDSP_OK;
      });
}

int pdsp_istft_host_f64(const double *re, const double *im, long long frames, long long fft_size, long long hop,
                        int window_type, double *out) {
  if (int rc = stft_host_checks(fft_size, hop, window_type)) return rc;
  if (frames < 1) return fail(PDSP_ERR_BAD_ARG, "frames must be >= 1, got %lld", frames);
  const long long bins = fft_size / 2 + 1;
  long long total = 0, in_count = 0;
  if (frames > 0x7fffffffLL || !mad_ok(frames - 1, hop, fft_size, &total) || total > (1LL << 40) ||
      !host_count_ok(frames, bins, &in_count))
    return fail(PDSP_ERR_BAD_ARG, "frames %lld x hop %lld overflows", frames, hop);
  if (!re || !im || !out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const size_t nin = (size_t)in_count, ny = (size_t)total;  // buffer: re | im | signal
  return packed_host_call(
      fft_size, window_type, 2 * nin + ny,
      [&](pdsp_plan *plan, hipStream_t s, const double *win, double *d) -> int {
        PDSP_HIP_TRY(hipMemcpyAsync(d, re, nin * sizeof(double), hipMemcpyHostToDevice, s));
        PDSP_HIP_TRY(hipMemcpyAsync(d + nin, im, nin * sizeof(double), hipMemcpyHostToDevice, s));
        return istft_t<double>(plan, frames, d, d + nin, hop, win, d + 2 * nin, s);
      },
      [&](const double *d) -> int {
        PDSP_HIP_TRY(hipMemcpy(out, d + 2 * nin, ny * sizeof(double), hipMemcpyDeviceToHost));
        return PDSP_OK;
      });
}

// pdsp_capi_fft2d.hip -- the 2-D transform of images (fft2 / ifft2, include/pdsp_hip_fft2d.h): the handle, entry points, host form.
// Host side only; calls fft2d_dev (pdsp_kernels_fft2d.hip).
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <new>

#include "pdsp_host.h"

using namespace pdsp_host;

/* ---- 2-D transform of images: fft2 / ifft2 (include/pdsp_hip_fft2d.h) --------- */

// A 2-D transform has no table of its own: the object borrows the cached plans of W and H points on its device and
// keeps them pinned while it lives (a pinned entry is never evicted and survives pdsp_plan_cache_clear), so every
// table it needs is on the device when create returns.  Built on TableHandle for the device and destroy_handle; its
// own lists of allocations stay empty.
struct pdsp_fft2d : TableHandle {
  long long h = 0, w = 0;
  CachedPlan plan_w, plan_h;
};

namespace {

int fft2d_shape(long long height, long long width, size_t elem, Fft2dPath *path) {
  if (fft2d_path(height, width, elem, path)) return PDSP_OK;
  return fail(PDSP_ERR_UNSUPPORTED_SIZE,
              "2-D FFT images must be H x W with H and W powers of two, 16 <= H <= 512, 16 <= W <= %d in f32 and %d in "
              "f64, got %lld x %lld (%d-byte scalars)",
              1 << pdsp::kMaxLog2N_f32, 1 << pdsp::kMaxLog2N_f64, height, width, (int)elem);
}

int check_fft2d_norm(int norm) {
  if (norm < PDSP_NORM_BACKWARD || norm > PDSP_NORM_FORWARD)
    return fail(PDSP_ERR_BAD_ARG, "2-D FFT norm must be 0 (backward), 1 (ortho) or 2 (forward), got %d", norm);
  return PDSP_OK;
}

// numpy's norm as the one scale of the last store, computed in f64 and rounded once (H W is a power of two: 1 / (H W)
// is exact, and 1 / sqrt(H W) is where log2(H W) is even)
double fft2d_scale(long long hw, int inverse, int norm) {
  if (norm == PDSP_NORM_ORTHO) return 1.0 / std::sqrt((double)hw);
  return (norm == PDSP_NORM_FORWARD) != (inverse != 0) ? 1.0 / (double)hw : 1.0;
}

// The argument checks of one call, ahead of the device; then the launch.  Exact in place is the one overlap allowed
// (the header's aliasing rule); the inverse is the forward transform of the swapped planes, so the rule is the same.
template <typename T>
int fft2d_t(const pdsp_fft2d *f, long long batch, const T *re_in, const T *im_in, T *re_out, T *im_out, int inverse,
            int norm, hipStream_t s) {
  if (!f) return fail(PDSP_ERR_BAD_ARG, "fft2d is null");
  if (batch < 1) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 1, got %lld", batch);
  if (int rc = check_fft2d_norm(norm)) return rc;
  if (!re_in || !re_out || !im_out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (inverse && !im_in) return fail(PDSP_ERR_BAD_ARG, "the inverse needs both planes (im_in is null)");
  Fft2dPath path;
  if (int rc = fft2d_shape(f->h, f->w, sizeof(T), &path)) return rc;
  long long count = 0;
  if (!mad_ok(batch, f->h * f->w, 0, &count) || count > (LLONG_MAX / 8))
    return fail(PDSP_ERR_BAD_ARG, "batch %lld x H x W overflows", batch);
  if ((((uintptr_t)re_in | (uintptr_t)im_in | (uintptr_t)re_out | (uintptr_t)im_out) & 15) != 0)
    return fail(PDSP_ERR_BAD_ARG, "the planes must begin on 16-byte boundaries");
  const size_t bytes = (size_t)count * sizeof(T);
  const bool in_place = re_out == re_in && (!im_in || im_out == im_in);
  if (!in_place && (host_ranges_overlap(re_out, bytes, re_in, bytes) || host_ranges_overlap(re_out, bytes, im_in, bytes) ||
                    host_ranges_overlap(im_out, bytes, re_in, bytes) || host_ranges_overlap(im_out, bytes, im_in, bytes)))
    return fail(PDSP_ERR_BAD_ARG, "output overlaps input (only re_out == re_in with im_out == im_in, or with a null "
                                  "im_in, may share bytes)");
  if (host_ranges_overlap(re_out, bytes, im_out, bytes))
    return fail(PDSP_ERR_BAD_ARG, "the output planes overlap each other");
  DeviceGuard dg(f->device);
  PDSP_HIP_TRY(dg.err);
  const T scale = (T)fft2d_scale(f->h * f->w, inverse, norm);
  if (inverse)
    return fft2d_dev<T>(path, f->plan_w.plan, f->plan_h.plan, batch, im_in, re_in, im_out, re_out, scale, s);
  return fft2d_dev<T>(path, f->plan_w.plan, f->plan_h.plan, batch, re_in, im_in, re_out, im_out, scale, s);
}

}  // namespace

int pdsp_fft2d_create(long long height, long long width, int device, pdsp_fft2d **out) {
  if (!out) return fail(PDSP_ERR_BAD_ARG, "out is null");
  Fft2dPath path;
  if (int rc = fft2d_shape(height, width, 4, &path)) return rc;  // the f32 domain holds the f64 one
  if (int rc = require_device()) return rc;
  if (int rc = resolve_device(&device)) return rc;
  DeviceGuard g(device);  // cached_plan asks for the current device's plans
  PDSP_HIP_TRY(g.err);
  HandleOwner<pdsp_fft2d> f(new (std::nothrow) pdsp_fft2d());
  if (!f) return fail(PDSP_ERR_BAD_ARG, "out of host memory");
  f->device = device, f->h = height, f->w = width;
  if (int rc = cached_plan(width, &f->plan_w)) return rc;
  if (int rc = cached_plan(height, &f->plan_h)) return rc;
  *out = f.release();
  return PDSP_OK;
}

int pdsp_fft2d_destroy(pdsp_fft2d *f) { return destroy_handle(f); }
long long pdsp_fft2d_height(const pdsp_fft2d *f) { return f ? f->h : 0; }
long long pdsp_fft2d_width(const pdsp_fft2d *f) { return f ? f->w : 0; }

int pdsp_fft2d_c2c_f32(const pdsp_fft2d *f, long long batch, const float *re_in, const float *im_in, float *re_out,
                       float *im_out, int inverse, int norm, pdsp_stream stream) {
  return fft2d_t<float>(f, batch, re_in, im_in, re_out, im_out, inverse, norm, (hipStream_t)stream);
}
int pdsp_fft2d_c2c_f64(const pdsp_fft2d *f, long long batch, const double *re_in, const double *im_in, double *re_out,
                       double *im_out, int inverse, int norm, pdsp_stream stream) {
  return fft2d_t<double>(f, batch, re_in, im_in, re_out, im_out, inverse, norm, (hipStream_t)stream);
}

int pdsp_fft2d_query(long long height, long long width, int scalar_bytes, int info[PDSP_FFT2D_INFO]) {
  if (!info) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (scalar_bytes != 4 && scalar_bytes != 8)
    return fail(PDSP_ERR_BAD_ARG, "scalar_bytes must be 4 or 8, got %d", scalar_bytes);
  Fft2dPath path;
  if (int rc = fft2d_shape(height, width, (size_t)scalar_bytes, &path)) return rc;
  info[0] = path.resident ? PDSP_FFT2D_RESIDENT : PDSP_FFT2D_TWO_PASS;
  info[1] = path.images, info[2] = path.tile, info[3] = path.launches;
  return PDSP_OK;
}

// The host form rides the packed features' scaffold on the cached plan of W points (its stream, its lock, its device).
// Its checks come in the stream entry points' order (batch, norm, buffers, then the shape).  The object lives for the
// call; it is made before the scaffold takes the W-plan's lock and destroyed after that lock is released, so no lock
// of the plan cache is ever taken under a plan's.  Buffer: re | im, transformed in place (a real image's zero plane is
// written here).
int pdsp_fft2d_host_f64(const double *re_in, const double *im_in, long long batch, long long height, long long width,
                        int inverse, int norm, double *re_out, double *im_out) {
  if (batch < 1) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 1, got %lld", batch);
  if (int rc = check_fft2d_norm(norm)) return rc;
  if (!re_in || !re_out || !im_out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (inverse && !im_in) return fail(PDSP_ERR_BAD_ARG, "the inverse needs both planes (im_in is null)");
  Fft2dPath path;
  if (int rc = fft2d_shape(height, width, sizeof(double), &path)) return rc;
  long long count = 0;
  if (batch > 0x7fffffffLL || !host_count_ok(batch, height * width, &count))
    return fail(PDSP_ERR_BAD_ARG, "batch %lld x (%lld, %lld) overflows", batch, height, width);
  const size_t n = (size_t)count;
  pdsp_fft2d *made = nullptr;
  if (int rc = pdsp_fft2d_create(height, width, -1, &made)) return rc;  // the current device: the scaffold's too
  const HandleOwner<pdsp_fft2d> own(made);
  const pdsp_fft2d *const f = made;
  return packed_host_call(
      width, PDSP_WIN_RECT, 2 * n,
      [&](pdsp_plan *, hipStream_t s, const double *, double *d) -> int {
        PDSP_HIP_TRY(hipMemcpyAsync(d, re_in, n * sizeof(double), hipMemcpyHostToDevice, s));
        if (im_in) PDSP_HIP_TRY(hipMemcpyAsync(d + n, im_in, n * sizeof(double), hipMemcpyHostToDevice, s));
        return fft2d_t<double>(f, batch, d, im_in ? d + n : nullptr, d, d + n, inverse, norm, s);
      },
      [&](const double *d) -> int {
        PDSP_HIP_TRY(hipMemcpy(re_out, d, n * sizeof(double), hipMemcpyDeviceToHost));
        PDSP_HIP_TRY(hipMemcpy(im_out, d + n, n * sizeof(double), hipMemcpyDeviceToHost));
        return PDSP_OK;
      });
}

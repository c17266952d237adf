// Kernel unit: the 2-D transform of images (pdsp_fft2d_kernel.h), f32 and f64.  See pdsp_internal.h.  The callers in
// pdsp_capi_fft2d.hip have validated every argument; `path` is fft2d_path()'s answer for this shape and precision.
#include "pdsp_internal.h"
#include "pdsp_fft2d_kernel.h"

namespace pdsp_host {

namespace {

template <typename T, int LH, int TILE>
hipError_t launch_cols_tile(const Tables<T> &th, long long blocks, T *re, T *im, long long w, T scale, long long batch,
                            hipStream_t s) {
  hipLaunchKernelGGL((pdsp::fft2d_cols_tile_kernel<T, LH, TILE>), dim3((unsigned)blocks), dim3(256), 0, s, re, im,
                     th.tw, (int)w, (int)(w / TILE), scale, batch);
  return hipGetLastError();
}

// The instantiations are fft2d_path()'s tiles: 64 columns at H = 64, 32 at H = 128, 32 (f32) / 16 (f64) at H = 256 and
// 512, and 16 where W = 16 (only H = 512 in f32: 256 x 16 is resident) or 32 where W = 32 caps a wider choice.
template <typename T>
hipError_t launch_cols(const Fft2dPath &path, int lh, const Tables<T> &th, long long blocks, T *re, T *im, long long w,
                       T scale, long long batch, hipStream_t s) {
  if (lh == 4 || lh == 5) {
    if (lh == 4) hipLaunchKernelGGL((pdsp::fft2d_cols_reg_kernel<T, 4>), dim3((unsigned)blocks), dim3(256), 0, s, re, im, (int)w, scale, batch);
    else hipLaunchKernelGGL((pdsp::fft2d_cols_reg_kernel<T, 5>), dim3((unsigned)blocks), dim3(256), 0, s, re, im, (int)w, scale, batch);
    return hipGetLastError();
  }
  if (lh == 6 && path.tile == 64) return launch_cols_tile<T, 6, 64>(th, blocks, re, im, w, scale, batch, s);
  if (lh == 7 && path.tile == 32) return launch_cols_tile<T, 7, 32>(th, blocks, re, im, w, scale, batch, s);
  if (lh == 9 && path.tile == 16) return launch_cols_tile<T, 9, 16>(th, blocks, re, im, w, scale, batch, s);
  if constexpr (sizeof(T) == 8) {
    if (lh == 8 && path.tile == 16) return launch_cols_tile<T, 8, 16>(th, blocks, re, im, w, scale, batch, s);
  } else {
    if (lh == 8 && path.tile == 32) return launch_cols_tile<T, 8, 32>(th, blocks, re, im, w, scale, batch, s);
    if (lh == 9 && path.tile == 32) return launch_cols_tile<T, 9, 32>(th, blocks, re, im, w, scale, batch, s);
  }
  return hipErrorInvalidValue;  // a tile fft2d_path() does not choose: no kernel is built for it
}

}  // namespace

template <typename T>
int fft2d_dev(const Fft2dPath &path, const pdsp_plan *plan_w, const pdsp_plan *plan_h, long long batch, const T *re_in,
              const T *im_in, T *re_out, T *im_out, T scale, hipStream_t s) {
  const int lh = plan_h->log2n, lw = plan_w->log2n;
  const long long h = plan_h->n, w = plan_w->n;
  const Tables<T> &tw = tables<T>(plan_w), &th = tables<T>(plan_h);
  if (path.resident) {
    const long long blocks = (batch + path.images - 1) / path.images;
    if (int rc = check_grid(blocks, batch)) return rc;
    const hipError_t e = with_int<4, 8>(lh, hipErrorInvalidValue, [&](auto LH) {
      return with_int<4, 8>(lw, hipErrorInvalidValue, [&](auto LW) {
        constexpr int A = decltype(LH)::value, B = decltype(LW)::value;
        if constexpr (A + B <= 12) {
          hipLaunchKernelGGL((pdsp::fft2d_resident_kernel<T, A, B>), dim3((unsigned)blocks), dim3(256), 0, s, re_in,
                             im_in, re_out, im_out, tw.tw, th.tw, scale, batch);
          return hipGetLastError();
        } else {
          return hipErrorInvalidValue;
        }
      });
    });
    PDSP_HIP_TRY(e);
    return PDSP_OK;
  }
  // rows: the W-plan's row kernels on batch * H rows, real or complex input into the output planes (the variant by
  // size alone, so that an image is transformed alike in every batch); then the columns in place, with the scale
  long long rows = 0, blocks = 0;
  if (!mad_ok(batch, h, 0, &rows) || !mad_ok(batch, w / path.tile, 0, &blocks))
    return fail(PDSP_ERR_BAD_ARG, "batch too large: %lld", batch);
  if (int rc = check_grid(blocks, batch)) return rc;
  if (int rc = run_complex<T>(plan_w, rows, re_in, im_in, re_out, im_out, T(1), s, true)) return rc;
  PDSP_HIP_TRY(launch_cols<T>(path, lh, th, blocks, re_out, im_out, w, scale, batch, s));
  return PDSP_OK;
}

template int fft2d_dev<float>(const Fft2dPath &, const pdsp_plan *, const pdsp_plan *, long long, const float *,
                              const float *, float *, float *, float, hipStream_t);
template int fft2d_dev<double>(const Fft2dPath &, const pdsp_plan *, const pdsp_plan *, long long, const double *,
                               const double *, double *, double *, double, hipStream_t);

}  // namespace pdsp_host

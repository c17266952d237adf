// Kernel unit: FIR filtering by fused overlap-save (pdsp_fir_kernel.h) and the filter spectrum, f32 and f64.
// See pdsp_internal.h.  The callers in pdsp_capi_fir.hip have validated every argument.
#include "pdsp_internal.h"
#include "pdsp_fir_kernel.h"

namespace pdsp_host {

template <typename T, int LOG2M>
static hipError_t launch_fir_one(bool fast, const T *x, long long len, long long x_stride, const T *h_re,
                                 const T *h_im, int p1, int hop, long long nblk, long long y_off, long long y_len, T *y,
                                 long long y_stride, const Tables<T> &t, long long items, hipStream_t s) {
  const T g = T(1) / T(4 << LOG2M);  // 1 / (2N)
  auto go = [&](auto fast_c) {
    hipLaunchKernelGGL((pdsp::fir_overlap_save_kernel<T, LOG2M, fast_c>), packed_grid<LOG2M>(items),
                       dim3(pdsp::kPackedWG<LOG2M>), 0, s, x, len, x_stride, h_re, h_im, p1, hop, nblk, y_off, y_len, y,
                       y_stride, t.tw_half, t.twr, g, items);
    return hipGetLastError();
  };
  return fast ? go(std::true_type{}) : go(std::false_type{});
}

template <typename T>
int fir_filter_dev(const pdsp_plan *plan, long long batch, const T *x, long long len, long long x_stride,
                   const T *h_re, const T *h_im, int p, long long y_off, long long y_len, T *y, long long y_stride,
                   long long nblk, hipStream_t s) {
  const Tables<T> &t = tables<T>(plan);
  const int log2m = plan->log2n - 1;
  const int p1 = p - 1, hop = (int)plan->n - p1;
  const long long items = batch * nblk;
  const bool fast = (((uintptr_t)x | (uintptr_t)y) & 7) == 0 && x_stride % 2 == 0 && y_stride % 2 == 0 && hop % 2 == 0 &&
                    (y_off - p1) % 2 == 0;
  const hipError_t e = with_int<5, 13>(log2m, hipErrorInvalidValue, [&](auto L) {
    return launch_fir_one<T, L>(fast, x, len, x_stride, h_re, h_im, p1, hop, nblk, y_off, y_len, y, y_stride, t, items, s);
  });
  PDSP_HIP_TRY(e);
  return PDSP_OK;
}

template <typename T>
int fir_spectrum_dev(const pdsp_plan *plan, const T *taps, int ntaps, T *h_re, T *h_im, hipStream_t s) {
  hipLaunchKernelGGL((pdsp::fir_spectrum_kernel<T>), dim3((unsigned)(plan->n / 2 + 1)), dim3(256), 0, s, taps, ntaps,
                     plan->log2n, h_re, h_im);
  PDSP_HIP_TRY(hipGetLastError());
  return PDSP_OK;
}

template int fir_filter_dev<float>(const pdsp_plan *, long long, const float *, long long, long long, const float *,
                                   const float *, int, long long, long long, float *, long long, long long, hipStream_t);
template int fir_filter_dev<double>(const pdsp_plan *, long long, const double *, long long, long long, const double *,
                                    const double *, int, long long, long long, double *, long long, long long, hipStream_t);
template int fir_spectrum_dev<float>(const pdsp_plan *, const float *, int, float *, float *, hipStream_t);
template int fir_spectrum_dev<double>(const pdsp_plan *, const double *, int, double *, double *, hipStream_t);

}  // namespace pdsp_host

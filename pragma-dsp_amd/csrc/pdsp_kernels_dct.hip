// Kernel unit: DCT-II and DCT-III of rows (pdsp_dct_kernel.h), f32 and f64.
// See pdsp_internal.h.  The callers in pdsp_capi_dct.hip have validated every argument.
#include "pdsp_internal.h"
#include "pdsp_dct_kernel.h"

namespace pdsp_host {

bool dct_fast_path(const void *x, long long x_stride, const void *y, long long y_stride, size_t elem) {
  return ((uintptr_t)x % 16 == 0) && ((uintptr_t)y % 16 == 0) && ((size_t)x_stride * elem) % 16 == 0 &&
         ((size_t)y_stride * elem) % 16 == 0;
}

template <typename T>
int dct_dev(const pdsp_plan *plan, long long batch, const T *x, long long x_stride, int type, T g, T g0, T *y,
            long long y_stride, hipStream_t s) {
  const Tables<T> &t = tables<T>(plan);
  const bool fast = dct_fast_path(x, x_stride, y, y_stride, sizeof(T));
  const hipError_t e = with_int<5, 13>(plan->log2n - 1, hipErrorInvalidValue, [&](auto L) {
    constexpr int LOG2M = decltype(L)::value;
    const dim3 grid = packed_grid<LOG2M>(batch), wg(pdsp::kPackedWG<LOG2M>);
    auto go = [&](auto fast_c) {
      if (type == 2)
        hipLaunchKernelGGL((pdsp::dct2_kernel<T, LOG2M, fast_c>), grid, wg, 0, s, x, x_stride, y, y_stride, t.tw_half,
                           t.twr, t.tw4n, g, g0, batch);
      else
        hipLaunchKernelGGL((pdsp::dct3_kernel<T, LOG2M, fast_c>), grid, wg, 0, s, x, x_stride, y, y_stride, t.tw_half,
                           t.twr, t.tw4n, g, g0, batch);
      return hipGetLastError();
    };
    return fast ? go(std::true_type{}) : go(std::false_type{});
  });
  PDSP_HIP_TRY(e);
  return PDSP_OK;
}

template int dct_dev<float>(const pdsp_plan *, long long, const float *, long long, int, float, float, float *,
                            long long, hipStream_t);
template int dct_dev<double>(const pdsp_plan *, long long, const double *, long long, int, double, double, double *,
                             long long, hipStream_t);

}  // namespace pdsp_host

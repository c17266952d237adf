// Kernel unit: the chirp-z transform and zoom FFT of rows (pdsp_czt_kernel.h), f32 and f64.
// See pdsp_internal.h.  The callers in pdsp_capi_chirp.hip have validated every argument.
#include "pdsp_internal.h"
#include "pdsp_czt_kernel.h"

namespace pdsp_host {

template <typename T>
int czt_dev(int log2m, long long len, long long bins, long long batch, const T *re_in, const T *im_in,
            long long in_stride, T *re_out, T *im_out, long long out_stride, const typename pdsp::vec2<T>::type *pre,
            const typename pdsp::vec2<T>::type *post, const typename pdsp::vec2<T>::type *bt,
            const typename pdsp::vec2<T>::type *tw, hipStream_t s) {
  const hipError_t e = with_int<5, 13>(log2m, hipErrorInvalidValue, [&](auto L) {
    constexpr int LOG2M = decltype(L)::value;
    hipLaunchKernelGGL((pdsp::czt_kernel<T, LOG2M>), packed_grid<LOG2M>(batch), dim3(pdsp::kPackedWG<LOG2M>), 0, s,
                       re_in, im_in, in_stride, (int)len, re_out, im_out, out_stride, (int)bins,
                       reinterpret_cast<const pdsp::cx<T> *>(pre), reinterpret_cast<const pdsp::cx<T> *>(post),
                       reinterpret_cast<const pdsp::cx<T> *>(bt), tw, batch);
    return hipGetLastError();
  });
  PDSP_HIP_TRY(e);
  return PDSP_OK;
}

template int czt_dev<float>(int, long long, long long, long long, const float *, const float *, long long, float *,
                            float *, long long, const float2 *, const float2 *, const float2 *, const float2 *,
                            hipStream_t);
template int czt_dev<double>(int, long long, long long, long long, const double *, const double *, long long, double *,
                             double *, long long, const double2 *, const double2 *, const double2 *, const double2 *,
                             hipStream_t);

}  // namespace pdsp_host

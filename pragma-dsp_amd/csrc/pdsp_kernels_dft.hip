// Kernel unit: the any-length DFT of rows by Bluestein's chirp-z algorithm (pdsp_bluestein_kernel.h), f32 and f64.
// See pdsp_internal.h.  The callers in pdsp_capi_chirp.hip have validated every argument.
#include "pdsp_internal.h"
#include "pdsp_bluestein_kernel.h"

namespace pdsp_host {

template <typename T>
int dft_dev(int log2m, long long len, long long batch, const T *re_in, const T *im_in, long long in_stride, T *re_out,
            T *im_out, long long out_stride, const typename pdsp::vec2<T>::type *chirp,
            const typename pdsp::vec2<T>::type *bt, const typename pdsp::vec2<T>::type *tw, bool inverse,
            hipStream_t s) {
  const T sgn = inverse ? T(-1) : T(1);
  const T g = inverse ? (T)(1.0 / (double)len) : T(1);
  const hipError_t e = with_int<5, 13>(log2m, hipErrorInvalidValue, [&](auto L) {
    constexpr int LOG2M = decltype(L)::value;
    hipLaunchKernelGGL((pdsp::bluestein_kernel<T, LOG2M>), packed_grid<LOG2M>(batch), dim3(pdsp::kPackedWG<LOG2M>), 0,
                       s, re_in, im_in, in_stride, (int)len, re_out, im_out, out_stride,
                       reinterpret_cast<const pdsp::cx<T> *>(chirp), reinterpret_cast<const pdsp::cx<T> *>(bt), tw, sgn,
                       g, batch);
    return hipGetLastError();
  });
  PDSP_HIP_TRY(e);
  return PDSP_OK;
}

template int dft_dev<float>(int, long long, long long, const float *, const float *, long long, float *, float *,
                            long long, const float2 *, const float2 *, const float2 *, bool, hipStream_t);
template int dft_dev<double>(int, long long, long long, const double *, const double *, long long, double *, double *,
                             long long, const double2 *, const double2 *, const double2 *, bool, hipStream_t);

}  // namespace pdsp_host

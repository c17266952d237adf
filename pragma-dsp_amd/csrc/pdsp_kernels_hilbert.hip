// Kernel unit: the Hilbert transform of rows and the analytic signal's parts (pdsp_hilbert_kernel.h), f32 and f64.
// See pdsp_internal.h.  The callers in pdsp_capi_hilbert.hip have validated every argument.
#include "pdsp_internal.h"
#include "pdsp_hilbert_kernel.h"

namespace pdsp_host {

static_assert(PDSP_HILBERT_ANALYTIC == pdsp::kHilbertAnalytic && PDSP_HILBERT_IMAG == pdsp::kHilbertImag &&
                  PDSP_HILBERT_ENVELOPE == pdsp::kHilbertEnvelope && PDSP_HILBERT_PHASE == pdsp::kHilbertPhase,
              "the kernel's mode switch reads pdsp_hilbert_out");

bool hilbert_fast_path(const void *x, long long x_stride, long long len, long long n, int out_mode, const void *y,
                       long long y_stride, size_t elem) {
  const size_t ya = out_mode == PDSP_HILBERT_ANALYTIC ? 16 : 2 * elem;
  return len == n && (uintptr_t)x % (2 * elem) == 0 && x_stride % 2 == 0 && (uintptr_t)y % ya == 0 &&
         ((size_t)y_stride * elem) % ya == 0;
}

template <typename T>
int hilbert_dev(const pdsp_plan *plan, long long batch, const T *x, long long x_stride, long long len, int out_mode,
                T *y, long long y_stride, hipStream_t s) {
  const Tables<T> &t = tables<T>(plan);
  const bool fast = hilbert_fast_path(x, x_stride, len, plan->n, out_mode, y, y_stride, sizeof(T));
  const hipError_t e = with_int<5, 13>(plan->log2n - 1, hipErrorInvalidValue, [&](auto L) {
    constexpr int LOG2M = decltype(L)::value;
    const T g = T(1) / T(4 << LOG2M);  // 1 / (2N)
    auto go = [&](auto fast_c) {
      hipLaunchKernelGGL((pdsp::hilbert_kernel<T, LOG2M, fast_c>), packed_grid<LOG2M>(batch),
                         dim3(pdsp::kPackedWG<LOG2M>), 0, s, x, (int)len, x_stride, out_mode, y, y_stride, t.tw_half,
                         t.twr, g, batch);
      return hipGetLastError();
    };
    return fast ? go(std::true_type{}) : go(std::false_type{});
  });
  PDSP_HIP_TRY(e);
  return PDSP_OK;
}

template int hilbert_dev<float>(const pdsp_plan *, long long, const float *, long long, long long, int, float *,
                                long long, hipStream_t);
template int hilbert_dev<double>(const pdsp_plan *, long long, const double *, long long, long long, int, double *,
                                 long long, hipStream_t);

}  // namespace pdsp_host

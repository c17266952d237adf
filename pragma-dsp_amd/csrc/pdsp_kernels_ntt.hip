// Kernel unit: the number-theoretic transform over GF(2^64 - 2^32 + 1), its inverse, the fused exact convolution and the
// element-wise product (pdsp_ntt_kernel.h).  See pdsp_internal.h.  The callers in pdsp_capi_ntt.hip have validated every
// argument.
#include "pdsp_internal.h"
#include "pdsp_ntt_kernel.h"

namespace pdsp_host {

template <int LOG2N, int OP>
static hipError_t ntt_launch(long long batch, const uint64_t *a, long long a_stride, int a_len, const uint64_t *b,
                             long long b_stride, int b_len, uint64_t *out, long long out_stride, int out_len,
                             const uint64_t *tw, hipStream_t s) {
  using TR = pdsp::NttTraits<LOG2N, OP>;
  auto *const k = &pdsp::ntt_kernel<LOG2N, OP>;
  if (TR::LDS_BYTES > 65536)  // beyond the default limit of dynamic LDS
    if (hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, 163840))
      return e;
  const unsigned blocks = (unsigned)((batch + TR::ROWS - 1) / TR::ROWS);
  hipLaunchKernelGGL(k, dim3(blocks), dim3(TR::WG), TR::LDS_BYTES, s, a, a_stride, a_len, b, b_stride, b_len, out,
                     out_stride, out_len, tw, batch);
  return hipGetLastError();
}

int ntt_dev(int log2n, int op, long long batch, const uint64_t *a, long long a_stride, int a_len, const uint64_t *b,
            long long b_stride, int b_len, uint64_t *out, long long out_stride, int out_len, const uint64_t *tw,
            hipStream_t s) {
  const hipError_t e = with_int<kNttMinLog2N, kNttMaxLog2N>(log2n, hipErrorInvalidValue, [&](auto l) {
    constexpr int L = decltype(l)::value;
    const auto go = [&](auto o) {
      return ntt_launch<L, decltype(o)::value>(batch, a, a_stride, a_len, b, b_stride, b_len, out, out_stride, out_len,
                                               tw, s);
    };
    switch (op) {
      case pdsp::NTT_FORWARD: return go(int_c<pdsp::NTT_FORWARD>{});
      case pdsp::NTT_INVERSE: return go(int_c<pdsp::NTT_INVERSE>{});
      case pdsp::NTT_CONV: return go(int_c<pdsp::NTT_CONV>{});
    }
    return hipErrorInvalidValue;
  });
  PDSP_HIP_TRY(e);
  return PDSP_OK;
}

template <int OP>
static long long ntt_blocks_op(int log2n, long long batch) {
  return with_int<kNttMinLog2N, kNttMaxLog2N>(log2n, batch, [&](auto l) {
    constexpr int R = pdsp::NttTraits<decltype(l)::value, OP>::ROWS;
    return (batch + R - 1) / R;
  });
}
long long ntt_blocks(int log2n, int op, long long batch) {
  return op == pdsp::NTT_CONV ? ntt_blocks_op<pdsp::NTT_CONV>(log2n, batch)
                              : ntt_blocks_op<pdsp::NTT_FORWARD>(log2n, batch);
}

int ntt_mul_dev(long long count, const uint64_t *a, const uint64_t *b, uint64_t *out, hipStream_t s) {
  hipLaunchKernelGGL(pdsp::ntt_mul_kernel, dim3(grid_for(count)), dim3(256), 0, s, a, b, out, count);
  PDSP_HIP_TRY(hipGetLastError());
  return PDSP_OK;
}

}  // namespace pdsp_host

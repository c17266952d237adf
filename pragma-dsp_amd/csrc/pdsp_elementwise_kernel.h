// pdsp_elementwise_kernel.h -- the stand-alone element-wise kernels: applyWindow, magnitude / phase, complex arithmetic.
#pragma once

#include <hip/hip_runtime.h>

namespace pdsp {

// ---- element-wise kernels (stand-alone applyWindow / magnitude / phase) -----

// `out` may be `in` (each index is read before it is written) and, in polar_kernel, `re` or `im`: those pointers
// carry no __restrict__.  The entry points refuse every other overlap.
template <typename T>
__global__ void __launch_bounds__(256)
apply_window_kernel(const T *in, const T *__restrict__ win, T *out, long long total, long long n) {
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step)
    out[i] = in[i] * win[i % n];
}

template <typename T, bool PHASE>
__global__ void __launch_bounds__(256)
polar_kernel(const T *re, const T *im, T *out, long long total) {
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
    const T a = re[i], b = im[i];
    if constexpr (PHASE) out[i] = T(atan2(b, a));
    else if constexpr (sizeof(T) == 8) out[i] = hypot(a, b);  // Math.hypot, fourier.ts:106 (range-safe)
    else {
      // f32: |x| within ~1e-19 .. 1e19 (header).  Both squares are exact in f64, so their sum is rounded to f32 once
      // (u) and the correctly rounded sqrt halves that and adds half an ulp: below 1 ulp in all.  Three f32 roundings
      // before the sqrt (2u) reach 1.5 ulp in the upper half of a binade (measured: 1.15 in 2^20 random pairs).
      out[i] = sqrt((float)((double)a * (double)a + (double)b * (double)b));
    }
  }
}

// Batched element-wise complex arithmetic on planar rows (src/math/complex.ts:26-197:
// add, sub, mul, div, conj, scale, mulScalar), so forward -> mul -> inverse pipelines
// (FFT-domain convolution, test/fluent/chain.test.ts:287-317) stay in HBM.  The second
// operand may be one row of `b_len` values broadcast over the batch (a filter response).
enum ComplexOp { kAdd = 0, kSub = 1, kMul = 2, kDiv = 3, kConj = 4, kScale = 5, kMulScalar = 6 };

// Every two-term sum is one explicit fma on one rounded product, and nothing else is contracted: left to the
// compiler, the V = 4 and V = 1 instantiations of complex_op_kernel fused different halves of mul and div, and a
// result depended in its last bit on the alignment of the operands.
template <typename T, int OP>
__device__ __forceinline__ void complex_op1(T ar, T ai, T br, T bi, T &orr, T &oi) {
#pragma clang fp contract(off)
  if constexpr (OP == kAdd) {
    orr = ar + br;
    oi = ai + bi;
  } else if constexpr (OP == kSub) {
    orr = ar - br;
    oi = ai - bi;
  } else if constexpr (OP == kMul || OP == kMulScalar) {  // (ac - bd) + i(ad + bc)
    const T p = ai * bi, q = ai * br;
    orr = fma(ar, br, -p);
    oi = fma(ar, bi, q);
  } else if constexpr (OP == kDiv) {  // ((ac + bd) + i(bc - ad)) / (c^2 + d^2), complex.ts:150-161
    const T dd = bi * bi, p = ai * bi, q = ar * bi;
    const T denom = fma(br, br, dd);
    orr = fma(ar, br, p) / denom;
    oi = fma(ai, br, -q) / denom;
  } else if constexpr (OP == kConj) {
    orr = ar;
    oi = -ai;
  } else {  // kScale: real scalar in br
    orr = ar * br;
    oi = ai * br;
  }
}

template <typename T, int V>
__device__ __forceinline__ void ld_vec(const T *p, long long i, T (&v)[V]) {
  if constexpr (V == 4) {
    typedef T V4 __attribute__((ext_vector_type(4)));
    const V4 t = reinterpret_cast<const V4 *>(p)[i];
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
    v[0] = p[i];
  }
}
template <typename T, int V>
__device__ __forceinline__ void st_vec(T *p, long long i, const T (&v)[V]) {
  if constexpr (V == 4) {
    typedef T V4 __attribute__((ext_vector_type(4)));
    reinterpret_cast<V4 *>(p)[i] = V4{v[0], v[1], v[2], v[3]};
  } else {
    p[i] = v[0];
  }
}

// No __restrict__: `out` may alias `a` (the fluent chain works in place) and `b` may be `out` too
// (chain.mul(chain)); every thread reads its own index of a and b before it writes that index.  A
// broadcast b (b_len < count) must not overlap `out`: pdsp_complex_op_f32 refuses that and every partial overlap.
template <typename T, int OP, int V>  // V values per thread per step (4 = 16-byte accesses)
__global__ void __launch_bounds__(256)
complex_op_kernel(const T *are, const T *aim, const T *bre, const T *bim, T sre, T sim, T *ore, T *oim,
                  long long count, long long b_len) {
  constexpr bool kBinary = OP <= kDiv;
  const long long nvec = count / V;
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += step) {
    T ar[V], ai[V], br[V], bi[V], orr[V], oi[V];
    ld_vec<T, V>(are, i, ar);
    ld_vec<T, V>(aim, i, ai);
    if constexpr (kBinary) {
      const long long j = b_len == count ? i : ((i * V) % b_len) / V;  // b_len % V == 0 on this path
      ld_vec<T, V>(bre, j, br);
      ld_vec<T, V>(bim, j, bi);
    }
#pragma unroll
    for (int v = 0; v < V; ++v)
      complex_op1<T, OP>(ar[v], ai[v], kBinary ? br[v] : sre, kBinary ? bi[v] : sim, orr[v], oi[v]);
    st_vec<T, V>(ore, i, orr);
    st_vec<T, V>(oim, i, oi);
  }
}

}  // namespace pdsp

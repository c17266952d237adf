// pdsp_goldilocks.h -- arithmetic in GF(p), p = 2^64 - 2^32 + 1, on the host and on the device: the one definition
// the NTT kernels (pdsp_ntt_kernel.h), the host-built twiddle table and the device-free helpers of the C ABI
// (pdsp_ntt_mulmod ...) share.  An element is a uint64_t; every function takes canonical values (< p) and returns one,
// canon() excepted, which takes any 64-bit pattern.  With eps = 2^32 - 1: 2^64 = eps and 2^96 = -1 (mod p), so 2 has
// order 192 and a product by a power of two is shifts.  Plain C++, no inline assembly.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PDSP_GL_FN __host__ __device__ __forceinline__
#else
#define PDSP_GL_FN inline
#endif

namespace pdsp {
namespace gl {

constexpr uint64_t kP = 0xffffffff00000001ULL;
constexpr uint64_t kEps = 0xffffffffULL;  // 2^64 mod p
constexpr uint64_t kGenerator = 7;        // generates the multiplicative group
constexpr int kMaxLog2Root = 32;          // p - 1 = 2^32 (2^32 - 1)

// any 64-bit pattern -> [0, p): 2^64 < 2 p, one conditional subtraction
PDSP_GL_FN uint64_t canon(uint64_t x) { return x >= kP ? x - kP : x; }

PDSP_GL_FN uint64_t sub(uint64_t a, uint64_t b) {
  uint64_t d;
  const bool borrow = __builtin_sub_overflow(a, b, &d);
  return d - (borrow ? kEps : 0);  // borrow: d = a - b + 2^64, wanted a - b + p
}

// a - (p - b): the same borrow rule (b = 0: a - p borrows and comes back as a)
PDSP_GL_FN uint64_t add(uint64_t a, uint64_t b) { return sub(a, kP - b); }

PDSP_GL_FN uint64_t neg(uint64_t a) { return a ? kP - a : 0; }

// lo + 2^64 hi (mod p), hi = hh 2^32 + hl: lo - hh + hl eps
PDSP_GL_FN uint64_t reduce128(uint64_t lo, uint64_t hi) {
  const uint64_t hh = hi >> 32, hl = hi & kEps;
  uint64_t t, r;
  if (__builtin_sub_overflow(lo, hh, &t)) t -= kEps;  // t + 2^64 - eps = t + p: no second borrow, lo >= 0 > hh - p
  const uint64_t m = (hl << 32) - hl;                 // hl eps < 2^64
  if (__builtin_add_overflow(t, m, &r)) r += kEps;    // the sum minus p
  return canon(r);
}

PDSP_GL_FN uint64_t mul(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return reduce128(a * b, __umul64hi(a, b));
#else
  const unsigned __int128 w = (unsigned __int128)a * b;
  return reduce128((uint64_t)w, (uint64_t)(w >> 64));
#endif
}

// x 2^s, 0 <= s < 192
PDSP_GL_FN uint64_t mul_pow2(uint64_t x, int s) {
  if (s >= 96) x = neg(x), s -= 96;
  if (s >= 64) x = reduce128(0, x), s -= 64;
  return s ? reduce128(x << s, x >> (64 - s)) : x;
}

PDSP_GL_FN uint64_t pow(uint64_t a, uint64_t e) {
  uint64_t r = 1;
  for (; e; e >>= 1, a = mul(a, a))
    if (e & 1) r = mul(r, a);
  return r;
}

// a^(p - 2); inv(0) = 0
PDSP_GL_FN uint64_t inv(uint64_t a) { return pow(a, kP - 2); }

// omega_N = 7^((p - 1) / N), N = 2^log2n, 0 <= log2n <= 32
PDSP_GL_FN uint64_t root(int log2n) { return pow(kGenerator, (kP - 1) >> log2n); }

}  // namespace gl
}  // namespace pdsp

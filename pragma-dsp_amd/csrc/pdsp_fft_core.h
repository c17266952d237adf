// pdsp_fft_core.h -- what the kernels are built from: single-pass, LDS-resident Stockham autosort FFT for gfx950.
//
// What it replaces: the body of Radix2Fft.transform, src/core/fft.ts:89-151 of
// pragma-dsp (bit-reversal scatter + log2 N radix-2 sweeps over memory + the
// inverse 1/N sweep), applied to `batch` independent rows, with the caller's
// pre/post element-wise steps (applyWindow, magnitude, phase, amplitude scaling:
// src/xform/fourier.ts:54-120, src/public/spectrum.ts:45-72) folded into the
// first load and the last store.  HBM is touched once each way; every butterfly
// stage runs out of registers and LDS.
//
// Shape: a transform is owned by TP = N/E threads with E points each in VGPRs.
// Pass p does radix-Rp butterflies in registers (log2 Rp radix-2 stages with
// compile-time constant twiddles), multiplies by the inter-pass twiddles
// W_{Ns*Rp}^{r*k} from a host-built f64->f32 table, and hands the points to the
// next pass through LDS in autosort order.  Global loads and stores are always
// `row*N + tid + TP*q` -- unit stride across the lanes of a wave -- so the
// bit-reversed scatter of the reference never happens in memory.
//
// Arithmetic: a complex point is ONE 2-wide vector register pair cx = (re, im), so
// complex add/sub, scaling and the two halves of a complex multiply are single
// v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32 instructions (swaps and sign flips ride
// on the op_sel / neg modifiers).  The N=16384 spectrum kernel is VALU-issue bound, so
// instruction count, not flops, is what this layout buys.
//
// No MFMA: an FFT is not a dense contraction (3.75 flop/B is far below the VALU roof).
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "pdsp_radix.h"

namespace pdsp {

// Diagnostic build only (tools/kbench -DPDSP_STAMPS): wave 0 of each workgroup adds the shader
// cycles between phase boundaries into pdsp_stamp_acc[slot]; nothing is emitted otherwise.
#ifdef PDSP_STAMPS
__device__ unsigned long long pdsp_stamp_acc[64];
#define PDSP_STAMP_INIT() unsigned long long stamp_last_ = clock64()
#define PDSP_STAMP(slot)                                                          \
  do {                                                                            \
    __builtin_amdgcn_sched_barrier(0);                                            \
    const unsigned long long t_ = clock64();                                      \
    if (threadIdx.x == 0) atomicAdd(&pdsp_stamp_acc[slot], t_ - stamp_last_);     \
    stamp_last_ = clock64();                                                      \
    __builtin_amdgcn_sched_barrier(0);                                            \
  } while (0)
#else
#define PDSP_STAMP_INIT() ((void)0)
#define PDSP_STAMP(slot) ((void)0)
#endif

template <typename T> struct vec2;
template <> struct vec2<float> { using type = float2; };
template <> struct vec2<double> { using type = double2; };

// A complex value as a native 2-wide vector: .x = re, .y = im.
template <typename T>
using cx = T __attribute__((ext_vector_type(2)));

template <int... Is, class F>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, Is...>, F &&f) {
  (f(std::integral_constant<int, Is>{}), ...);
}
// Fully unrolled loop whose index is a compile-time constant (register arrays
// must never be indexed at run time: they would go to scratch).
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
  static_for_impl(std::make_integer_sequence<int, N>{}, static_cast<F &&>(f));
}

constexpr int ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}
constexpr int bitrev(int x, int bits) {
  int y = 0;
  for (int b = 0; b < bits; ++b) {
    y = (y << 1) | (x & 1);
    x >>= 1;
  }
  return y;
}

// Empty asm that claims to modify every element: the values become opaque at this point (keeps loads
// from sinking past it in the stamped build; keeps loop-invariant values from being hoisted with
// everything derived from them in the multi-frame kernels).
template <typename T, int E, int I = 0>
__device__ __forceinline__ void pin_regs(T __attribute__((ext_vector_type(2))) (&a)[E]) {
  if constexpr (I < E) {
    asm volatile("" : "+v"(a[I]));
    pin_regs<T, E, I + 1>(a);
  }
}

// ---- complex helpers on cx ---------------------------------------------------

template <typename T>
__device__ __forceinline__ cx<T> mul_neg_i(const cx<T> a) {  // a * (-i) = (im, -re)
  return cx<T>{a.y, -a.x};
}
template <typename T>
__device__ __forceinline__ cx<T> conj(const cx<T> a) {
  return cx<T>{a.x, -a.y};
}
// a + (-i)*b = (a.re + b.im, a.im - b.re)  and  a + i*b = (a.re - b.im, a.im + b.re): ONE v_pk_fma_f32 each, since
// hipcc folds the half swap of fma(b.yx, (1, -1), a) into op_sel (exact).  Plain arithmetic materialises (-i)*b first;
// the inline-asm v_pk_add_f32 of rounds 1-2 cost an s_nop pad per statement (68 of 673 instructions at N=4096).
template <typename T>
__device__ __forceinline__ cx<T> add_mul_neg_i(const cx<T> a, const cx<T> b) {
  if constexpr (std::is_same_v<T, float>) {
    return __builtin_elementwise_fma(__builtin_shufflevector(b, b, 1, 0), cx<float>{1.0f, -1.0f}, a);
  } else {
    return cx<T>{a.x + b.y, a.y - b.x};
  }
}
template <typename T>
__device__ __forceinline__ cx<T> add_mul_pos_i(const cx<T> a, const cx<T> b) {
  if constexpr (std::is_same_v<T, float>) {
    return __builtin_elementwise_fma(__builtin_shufflevector(b, b, 1, 0), cx<float>{-1.0f, 1.0f}, a);
  } else {
    return cx<T>{a.x - b.y, a.y + b.x};
  }
}
// a * w = a.re*(w.re, w.im) + a.im*(-w.im, w.re): one pk_mul + one pk_fma (f32: spelled out for the
// same reason -- the second product's swapped, half-negated operand is an op_sel / neg_lo pattern)
template <typename T>
__device__ __forceinline__ cx<T> cmul(const cx<T> a, const cx<T> w) {
  if constexpr (std::is_same_v<T, float>) {
    // both instructions in ONE statement (the product accumulates in the result register): half the asm boundaries
    // for hipcc to pad, one register less than two statements
    cx<float> r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1]\n\t"
        "v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]"
        : "=&v"(r)
        : "v"(a), "v"(w));
    return r;
  } else {
    return a.xx * w + a.yy * cx<T>{-w.y, w.x};
  }
}

// a * W16^M,  W16 = e^{-2*pi*i/16},  0 <= M < 8.
template <typename T, int M>
__device__ __forceinline__ cx<T> mul_w16(const cx<T> a) {
  constexpr T C1 = T(0.92387953251128673848);  // cos(pi/8)
  constexpr T C2 = T(0.70710678118654752440);  // cos(pi/4)
  constexpr T C3 = T(0.38268343236508977173);  // sin(pi/8)
  if constexpr (M == 0) {
    return a;
  } else if constexpr (M == 4) {  // -i
    return mul_neg_i(a);
  } else if constexpr (M == 2) {  // (1 - i)/sqrt2: (re + im, im - re) * C2
    return add_mul_neg_i(a, a) * C2;
  } else if constexpr (M == 6) {  // (-1 - i)/sqrt2 = -(1 + i)/sqrt2: -(re - im, im + re) * C2
    return add_mul_pos_i(a, a) * (-C2);
  } else {
    constexpr T c = M == 1 ? C1 : M == 3 ? C3 : M == 5 ? -C3 : -C1;
    constexpr T s = M == 1 ? -C3 : M == 3 ? -C1 : M == 5 ? -C1 : -C3;  // W = c + i*s
    return a.xx * cx<T>{c, s} + a.yy * cx<T>{-s, c};
  }
}

template <typename T, int NUM>
__device__ __forceinline__ cx<T> mul_w32(const cx<T> a);

// In-register radix-R DFT (R = 2, 4, 8, 16; 32 for whole tiny rows) as log2 R decimation-in-frequency
// radix-2 stages -- each one a stage of the reference's loop nest
// (src/core/fft.ts:116-140) with a compile-time twiddle.  Output k lands in slot bitrev(k).
// Radix-4 DIF butterfly on four registers, outputs in natural order y0..y3.  The two odd outputs are
// (x0 - x2) -/+ i (x1 - x3): one fused add each, no materialised rotation.
template <typename T>
__device__ __forceinline__ void bfly4(cx<T> &a0, cx<T> &a1, cx<T> &a2, cx<T> &a3) {
  const cx<T> t0 = a0 + a2, t1 = a0 - a2, t2 = a1 + a3, t3 = a1 - a3;
  a0 = t0 + t2;
  a2 = t0 - t2;
  a1 = add_mul_neg_i(t1, t3);
  a3 = add_mul_pos_i(t1, t3);
}
// The same with input x2 still carrying a pending factor -i (x2 = -i * d): t0 = x0 - i d, t1 = x0 + i d.
template <typename T>
__device__ __forceinline__ void bfly4_x2_rot(cx<T> &a0, cx<T> &a1, cx<T> &d, cx<T> &a3) {
  const cx<T> t0 = add_mul_neg_i(a0, d), t1 = add_mul_pos_i(a0, d), t2 = a1 + a3, t3 = a1 - a3;
  a0 = t0 + t2;
  d = t0 - t2;
  a1 = add_mul_neg_i(t1, t3);
  a3 = add_mul_pos_i(t1, t3);
}

template <typename T, int R>
__device__ __forceinline__ void fft_reg(cx<T> (&a)[R]) {
  static_assert(R >= 1 && R <= 32 && (R & (R - 1)) == 0, "radix");
  if constexpr (R == 4) {
    bfly4(a[0], a[1], a[2], a[3]);  // X[q] in slot q; bitrev order wants X[1] <-> X[2] swapped
    const cx<T> x1 = a[1];
    a[1] = a[2];
    a[2] = x1;
    return;
  } else if constexpr (R == 8) {
    // one radix-2 step (W8^k on the odd half; W8^2 = -i stays pending), then a radix-4 on each half
    static_for<4>([&](auto kc) {
      constexpr int k = kc;
      const cx<T> u = a[k], v = a[k + 4];
      a[k] = u + v;
      if constexpr (k == 2) a[k + 4] = u - v;  // times -i inside bfly4_x2_rot
      else a[k + 4] = mul_w32<T, 4 * k>(u - v);
    });
    bfly4(a[0], a[1], a[2], a[3]);            // X[2m] in a[m]
    bfly4_x2_rot(a[4], a[5], a[6], a[7]);     // X[2m+1] in a[4+m]
    cx<T> o[8];
    static_for<8>([&](auto kc) {
      constexpr int k = kc;
      o[bitrev(k, 3)] = a[(k & 1) * 4 + (k >> 1)];
    });
    static_for<8>([&](auto kc) { a[kc] = o[kc]; });
    return;
  } else if constexpr (R == 16) {
    // two radix-4 stages: 64 fused adds + 8 twiddle products, no rotation is ever materialised.
    // Stage A over stride 4: y_q of column j lands in a[j + 4q], then times W16^(j*q).
    static_for<4>([&](auto jc) {
      constexpr int j = jc;
      bfly4(a[j], a[j + 4], a[j + 8], a[j + 12]);
      if constexpr (j > 0) {
        a[j + 4] = mul_w32<T, 2 * j>(a[j + 4]);                           // W16^j
        if constexpr (j != 2) a[j + 8] = mul_w32<T, (4 * j) % 32>(a[j + 8]);  // W16^2j (j = 2: the -i stays pending)
        a[j + 12] = mul_w32<T, (6 * j) % 32>(a[j + 12]);                  // W16^3j
      }
    });
    // Stage B on each group of four: X[q + 4*q2] lands in a[4q + q2]
    bfly4(a[0], a[1], a[2], a[3]);
    bfly4(a[4], a[5], a[6], a[7]);
    bfly4_x2_rot(a[8], a[9], a[10], a[11]);  // a[10] = y_2 of column 2, still to be multiplied by W16^4 = -i
    bfly4(a[12], a[13], a[14], a[15]);
    // callers expect output k in slot bitrev(k, 4)
    cx<T> o[16];
    static_for<16>([&](auto kc) {
      constexpr int k = kc;
      o[bitrev(k, 4)] = a[4 * (k & 3) + (k >> 2)];
    });
    static_for<16>([&](auto kc) { a[kc] = o[kc]; });
    return;
  }
  static_for<ilog2(R)>([&](auto stc) {
    constexpr int s = R >> (stc + 1);  // half length of this stage's sub-transforms
    static_for<R / 2>([&](auto ic) {
      constexpr int g = (ic / s) * 2 * s, k = ic % s;
      constexpr int i0 = g + k, i1 = i0 + s;
      const cx<T> u = a[i0], v = a[i1];
      a[i0] = u + v;
      a[i1] = mul_w32<T, k *(16 / s)>(u - v);  // W_{2s}^k (even multiples resolve to the W16 forms)
    });
  });
}

template <int LOG2N, int LOG2E = 4>
struct FftTraits {
  static constexpr RadixPlan P = make_radix_plan(LOG2N, LOG2E);
  static constexpr int N = P.n, E = P.e, TP = P.tp, NP = P.np;
  static constexpr int WG = TP >= 256 ? TP : 256;  // threads per workgroup
  static constexpr int ROWS = WG / TP;             // transforms per workgroup
  // one pad element every 16: the radix-16 scatter (stride 16 complex) would
  // otherwise put a whole ds_write lane group on one bank
  static constexpr int LROW = N + N / 16;
  static constexpr int LDS_ELEMS = NP > 1 ? ROWS * LROW : 1;
};

// threads per workgroup of the packed-real kernels (sixteen points per thread: PackedRow)
template <int LOG2M>
constexpr int kPackedWG = FftTraits<LOG2M>::WG;

__device__ __forceinline__ int lds_pad(int i) { return i + (i >> 4); }
// pad(a + c) == pad(a) + cpad(c) when c is a multiple of 16 (or a is and c < 16)
constexpr int cpad(int c) { return c + c / 16; }

// Bank conflicts of this layout, measured where the SQ counters do not saturate (2,048 rows per launch;
// profiles/r03_lds_bank_conflicts_unsaturated.txt): the pad keeps the radix-16 SCATTER (ds_write_b64: 16-lane groups
// over 32 banks) conflict-free but costs every READ-BACK a 2-way conflict -- a ds_read_b64 is served in two groups of
// 32 lanes over 64 banks, and 32 consecutive points of a padded row span 33 slots, so lanes 0 and 31 of each group
// meet on one bank pair: SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = exactly 0.25 on fft_stockham_kernel<12> (64 of
// 256 LDS-array cycles per wave), 0.20 on spectrum_dif16k_kernel.  No additive pad that is constant over 16-point
// blocks can serve both sides (the scatter needs the pads of blocks 2s and 2s+1 to differ mod 16, the read-back
// needs them equal mod 32).  An XOR swizzle, i ^ ((i >> 4) & 15), does -- built in round 3 for configs[2]'s kernel:
// conflicts 524,288 -> 0 and LDS-array cycles -25 % per launch, at +59 vector instructions per thread (the
// scatter's addresses are no longer base + constant) and 97 instead of 70 VGPRs; time 0.6681 vs 0.6689 ms, board
// power 1,390 vs 1,388 W (tools' one-process A/B, profiles/r03_experiments/ab_lds_swizzle_*): the conflict cycles
// are neither on the critical path nor in the power budget of an HBM-bound kernel, so the padded form stays and
// the swizzled one was removed again.
// A transform owned by >= 64 threads has one row per wave: tell the compiler the row
// is wave-uniform so row bases live in SGPRs (batch < 2^31 is checked on the host).
template <int TP>
__device__ __forceinline__ long long uniform_row(long long row) {
  if constexpr (TP >= 64) return (long long)__builtin_amdgcn_readfirstlane((int)row);
  else return row;
}

// Order of a kernel's first loads.  The memory counter retires in issue order, so table loads issued behind a row's
// HBM loads wait for all of them.  The spectrum and split kernels request their L2-resident tables (twiddle bases,
// split twiddles, window values) BEFORE the streamed row: packed kernel +1 ... +4 %, N=16384 spectrum 5.07 -> 5.40
// TB/s, N=16384 complex +2 ... 7 %.  The plain transforms (fft_stockham_kernel, fft_real_kernel), whose only tables
// are 12-14 twiddle bases, lose 1-3.5 % that way and load them behind the row ("Tables first").
__device__ __forceinline__ void load_order_fence() { __builtin_amdgcn_sched_barrier(0); }

// Streamed rows are touched exactly once: non-temporal loads/stores keep them from
// displacing the twiddle/window tables in L2 (+4..10 % on the row-pattern copy and on
// the C2C kernel, tools/kbench).
template <typename T>
__device__ __forceinline__ T ld_stream(const T *p) { return __builtin_nontemporal_load(p); }
template <typename T>
__device__ __forceinline__ void st_stream(T v, T *p) { __builtin_nontemporal_store(v, p); }
// Amplitude / phase rows of dword stores take plain stores: they are N/2+1 floats long, so a wave's 256-byte store
// straddles cache lines that the neighbouring waves complete, and L2 combines plain stores
// (PMC: non-temporal stores wrote 13 % more than the algorithmic bytes here).

// |z| for the fused amplitude stores: one v_sqrt_f32 (1 ulp) instead of the ~10-instruction
// correctly rounded sequence -- 17 of them per thread sit in the VALU-bound epilogue of the
// N=16384 spectrum kernel.  1 ulp = 6e-8 relative, far inside the 1e-5 contract.
__device__ __forceinline__ float mag(const cx<float> z) {
  const cx<float> s = z * z;
  return __builtin_amdgcn_sqrtf(s.x + s.y);
}
// f64 is the drop-in's default arithmetic and the reference's magnitude() is Math.hypot
// (src/xform/fourier.ts:106): no overflow above 1e154, no underflow below 1e-162.
// (Round 3 tried sqrt(fma(re, re, im * im)) with hypot only outside [2^-900, 2^1000]: the fast path is ~15 f64
// instructions against hypot's ~35, 17 times per thread -- and the f64 spectrum sweep moved by +4 % at N = 1024,
// +-1 % at 2048 ... 8192 and -6 ... -8 % at N = 128 ... 512: no gain, hypot stays.
// profiles/r03_experiments/sweep_f64_hypot_vs_fastmag.txt)
__device__ __forceinline__ double mag(const cx<double> z) { return hypot(z.x, z.y); }

// Eight consecutive values of a cosine-sum window (createWindow, fourier.ts:14-52) by angle addition, two per
// packed instruction: c0 = (cos t, sin t) of the first sample, we[e] = (cos f e, sin f e) wave-uniform;
// w[e] = k0 + k1 cos(t + f e), or k0 + c (k1 + k2 c) for the three-term window (cos 2t = 2 c^2 - 1 folded in).
template <typename T, bool THREE>
__device__ __forceinline__ void fused_window_pairs(const cx<T> c0, const cx<T> *__restrict__ we, const T k0, const T k1,
                                                   const T k2, cx<T> (&w)[4]) {
  static_for<4>([&](auto h) {
    const cx<T> e0 = we[2 * h], e1 = we[2 * h + 1];
    const cx<T> c = cx<T>{e0.x, e1.x} * c0.x - cx<T>{e0.y, e1.y} * c0.y;  // cos(t + f e), e = 2h, 2h + 1
    if constexpr (THREE) w[h] = c * (c * k2 + k1) + k0;
    else w[h] = c * k1 + k0;
  });
}

// ---- twiddle providers ---------------------------------------------------------
// twf.template get<p, r, b>(j) = W_{Ns*R}^{r*(j mod Ns)} for input r of butterfly j = tid + b*TP of pass p.

// Reads the host-built table (layout: pdsp_radix.h) at every use: uniform table base per r
// (SGPR) + one 32-bit lane offset k.
template <typename T, int LOG2N, int LOG2E = 4>
struct TableTwiddles {
  const cx<T> *__restrict__ tw;
  template <int p, int r, int b>
  __device__ __forceinline__ cx<T> get(const int j) const {
    using TR = FftTraits<LOG2N, LOG2E>;
    constexpr int Ns = TR::P.ns[p];
    return (tw + (TR::P.twoff[p] + (r - 1) * Ns))[(unsigned)(j & (Ns - 1))];
  }
};

// a * e^{-2*pi*i*NUM/32}, NUM compile-time
template <typename T, int NUM>
__device__ __forceinline__ cx<T> mul_w32(const cx<T> a) {
  constexpr int m = ((NUM % 32) + 32) % 32;
  if constexpr (m % 2 == 0) {
    constexpr int h = m / 2;  // W16^h
    if constexpr (h >= 8) return -mul_w16<T, h - 8>(a);
    else return mul_w16<T, h>(a);
  } else {
    // cos(pi*q/16), q = 0..8
    constexpr double C[9] = {1.0, 0.98078528040323044913, 0.92387953251128675613, 0.83146961230254523708,
                             0.70710678118654752440, 0.55557023301960222474, 0.38268343236508977173,
                             0.19509032201612826785, 0.0};
    constexpr int q = m % 16;
    constexpr bool neg = m >= 16;
    constexpr int lo = q <= 8 ? q : 16 - q;  // fold onto the first quarter turn
    constexpr double cq = q <= 8 ? C[lo] : -C[lo];
    constexpr double sq = C[8 - lo];
    constexpr T c = T(neg ? -cq : cq), s = T(neg ? sq : -sq);  // W = c + i*s
    return a.xx * cx<T>{c, s} + a.yy * cx<T>{-s, c};
  }
}

// a * e^{-2*pi*i*NUM/64}, NUM compile-time
template <typename T, int NUM>
__device__ __forceinline__ cx<T> mul_w64(const cx<T> a) {
  static_assert(NUM >= 0 && NUM < 64, "one turn");
  if constexpr (NUM >= 32) {
    return -mul_w64<T, NUM - 32>(a);
  } else if constexpr (NUM % 2 == 0) {
    return mul_w32<T, NUM / 2>(a);
  } else {
    // cos(pi*j/32), j = 0..16
    constexpr double C[17] = {1.0,
                              0.99518472667219688624, 0.98078528040323044913, 0.95694033573220886494,
                              0.92387953251128675613, 0.88192126434835502971, 0.83146961230254523708,
                              0.77301045336273696081, 0.70710678118654752440, 0.63439328416364549822,
                              0.55557023301960222474, 0.47139673682599764856, 0.38268343236508977173,
                              0.29028467725446236764, 0.19509032201612826785, 0.09801714032956060199,
                              0.0};
    constexpr int lo = NUM <= 16 ? NUM : 32 - NUM;  // fold onto the first quarter turn
    constexpr double cq = NUM <= 16 ? C[lo] : -C[lo];
    constexpr double sq = C[16 - lo];
    constexpr T c = T(cq), s = T(-sq);  // W = cos - i sin
    return a.xx * cx<T>{c, s} + a.yy * cx<T>{-s, c};
  }
}

// Per-thread twiddle BASES held in registers.  A thread's twiddles depend only on its
// position in the transform, so they are fetched once, right behind the frame loads (their
// L2 latency hides under the HBM wait) instead of inside every pass, where a stamped build
// showed each table fetch exposed for thousands of cycles behind the streaming traffic.
// Per radix-16 pass six bases {w, w^2, w^3, w^4, w^8, w^12} of the thread's own k; the other
// nine are one product of two table-exact values.  A short last pass (Ns > TP) needs only
// k = tid: W_N^{r*(tid + b*TP)} = base_r * W16^{r*b} because TP = N/16.
template <typename T, int LOG2N, int LOG2E = 4>
struct RegTwiddles {
  using TR = FftTraits<LOG2N, LOG2E>;
  static_assert(LOG2E == 4, "the W16 correction of the short last pass assumes TP = N/16");
  static constexpr int nb(int p) { return TR::P.ns[p] > 1 ? (TR::P.r[p] == 16 ? 6 : TR::P.r[p] - 1) : 0; }
  static constexpr int off(int p) {
    int o = 0;
    for (int i = 0; i < p; ++i) o += nb(i);
    return o;
  }
  static constexpr int TOTAL = off(TR::NP) > 0 ? off(TR::NP) : 1;
  // which power r the i-th base of a radix-R pass holds: 16 -> 1,2,3,4,8,12; else 1..R-1
  static constexpr int base_r(int R, int i) { return R == 16 ? (i < 4 ? i + 1 : (i - 2) * 4) : i + 1; }

  cx<T> tb[TOTAL];

  __device__ __forceinline__ void load(const cx<T> *__restrict__ tw, const int tid) {
    static_for<TR::NP>([&](auto pc) {
      constexpr int p = pc;
      constexpr int Ns = TR::P.ns[p], R = TR::P.r[p];
      if constexpr (Ns > 1) {
        // Ns <= TP for every pass but a short last one, where j = tid + b*TP < Ns
        const unsigned k0 = (unsigned)(Ns <= TR::TP ? (tid & (Ns - 1)) : tid);
        static_for<nb(p)>([&](auto ic) {
          constexpr int r = base_r(R, ic);
          tb[off(p) + ic] = (tw + (TR::P.twoff[p] + (r - 1) * Ns))[k0];
        });
      }
    });
  }

  template <int p, int r, int b>
  __device__ __forceinline__ cx<T> get(const int) const {
    constexpr int Ns = TR::P.ns[p], R = TR::P.r[p], O = off(p);
    cx<T> w;
    if constexpr (R == 16) {
      constexpr int hi = r & 12, lo = r & 3;
      if constexpr (hi == 0) w = tb[O + lo - 1];
      else if constexpr (lo == 0) w = tb[O + 2 + hi / 4];
      else w = cmul(tb[O + 2 + hi / 4], tb[O + lo - 1]);  // w^(hi+lo) = w^hi * w^lo
    } else {
      w = tb[O + r - 1];
    }
    if constexpr (Ns > TR::TP && b > 0) w = mul_w32<T, 2 * ((r * b) % 16)>(w);  // * W16^{r*b}
    return w;
  }
};

// ---- the passes --------------------------------------------------------------

// Pass p for one thread's E points: twiddle, radix-R butterflies, then either the autosort scatter
// to LDS or (register-resident last pass) back into x in natural order.
template <typename T, int LOG2N, bool LAST_TO_LDS, int LOG2E, int p, class TWF, int EE>
__device__ __forceinline__ void fft_pass_compute(cx<T> (&x)[EE], cx<T> *const lrow, const TWF &twf, const int tid) {
  using TR = FftTraits<LOG2N, LOG2E>;
  constexpr int E = TR::E, TP = TR::TP, NP = TR::NP;
  static_assert(EE == E, "register array size must be the plan's points per thread");
  // For N >= 256 every LDS address is (a thread-only base) + (a compile-time offset),
  // so there is one address register per pass instead of one per element.
  constexpr bool kConstOffsets = (TP % 16 == 0);
  constexpr int R = TR::P.r[p], Ns = TR::P.ns[p], EB = E / R, LR = ilog2(R);
  constexpr bool last = (p == NP - 1);
  constexpr bool to_lds = !last || LAST_TO_LDS;

  static_for<EB>([&](auto bc) {
    constexpr int b = bc;
    cx<T> a[R];
    static_for<R>([&](auto rc) { a[rc] = x[b + rc * EB]; });
    const int j = tid + b * TP;  // butterfly index within the pass, 0 <= j < N/R
    if constexpr (Ns > 1) {
      static_for<R - 1>([&](auto rc) {
        constexpr int r = rc + 1;
        a[r] = cmul(a[r], twf.template get<p, r, b>(j));
      });
    }
    fft_reg<T, R>(a);
    if constexpr (!to_lds) {
      // Ns*R == N: output r of butterfly j is X[j + r*N/R] = slot b + r*EB
      static_for<R>([&](auto rc) { x[b + rc * EB] = a[bitrev(rc, LR)]; });
    } else if constexpr (kConstOffsets) {
      // autosort scatter (natural order when Ns*R == N).  j = tid + b*TP: the part of the
      // index that depends on b and rc is the constant c = cb + rc*Ns, and
      // pad(j0t + c) == pad(j0t) + cpad(c): cb is a multiple of 16, and (j0t & 15) + (rc*Ns & 15)
      // never carries (for Ns < 16 the first is < Ns, the second a multiple of Ns below 16)
      constexpr int cb = Ns <= TP ? b * TP * R : b * TP;
      const int j0t = Ns <= TP ? ((tid >> ilog2(Ns)) << ilog2(Ns * R)) + (tid & (Ns - 1)) : tid;
      cx<T> *const wbase = lrow + lds_pad(j0t);
      static_for<R>([&](auto rc) { wbase[cpad(cb + rc * Ns)] = a[bitrev(rc, LR)]; });
    } else {
      const int j0 = ((j >> ilog2(Ns)) << ilog2(Ns * R)) + (j & (Ns - 1));
      static_for<R>([&](auto rc) { lrow[lds_pad(j0 + rc * Ns)] = a[bitrev(rc, LR)]; });
    }
  });
}

// The thread's E inputs of the next pass, x[q] = row[tid + TP*q], after the barrier behind a scatter.
template <typename T, int LOG2N, int LOG2E, int EE>
__device__ __forceinline__ void fft_pass_readback(cx<T> (&x)[EE], const cx<T> *const lrow, const int tid) {
  using TR = FftTraits<LOG2N, LOG2E>;
  constexpr int E = TR::E, TP = TR::TP;
  // (For TP <= 128 hipcc pairs these read-backs into ds_read2_b64, which the LDS serves at half ds_read_b64's rate.
  // Keeping them apart -- round-robin opaque bases, +4 instructions -- measured +-0 on every size from 256 to 8192,
  // C2C and fused spectrum (profiles/r03_experiments/ab_lds_read2_vs_split.log): LDS time is not what bounds these
  // kernels, same finding as the bank-conflict experiment at lds_pad.)
  if constexpr (TP % 16 == 0) {
    const cx<T> *const rbase = lrow + lds_pad(tid);
    static_for<E>([&](auto q) { x[q] = rbase[cpad(TP * q)]; });
  } else {
    static_for<E>([&](auto q) { x[q] = lrow[lds_pad(tid + TP * q)]; });
  }
}

// Runs every pass of the length-2^LOG2N transform on the E points each of the TP
// cooperating threads holds.  LAST_TO_LDS = false: the result comes back in the
// registers, X[tid + TP*q] in slot q.  LAST_TO_LDS = true: the last pass also
// scatters to LDS, in natural order (X[k] at lds_pad(k)), for a consumer that needs
// other threads' bins; the caller must __syncthreads() before reading it.
// Inter-pass twiddles W_{Ns*R}^{r*k} come from the provider `twf` (table or registers).
template <typename T, int LOG2N, bool LAST_TO_LDS, int LOG2E = 4, class TWF = void, int EE = 0>
__device__ __forceinline__ void fft_passes(cx<T> (&x)[EE], cx<T> *const lrow, const TWF &twf, const int tid) {
  PDSP_STAMP_INIT();
  constexpr int NP = FftTraits<LOG2N, LOG2E>::NP;
  static_for<NP>([&](auto pc) {
    constexpr int p = pc;
    fft_pass_compute<T, LOG2N, LAST_TO_LDS, LOG2E, p>(x, lrow, twf, tid);
    PDSP_STAMP(8 + 4 * p);  // twiddle loads + butterflies + LDS scatter issued
    if constexpr (p != NP - 1) {
      __syncthreads();
      PDSP_STAMP(9 + 4 * p);  // barrier (incl. draining the scatter)
      fft_pass_readback<T, LOG2N, LOG2E>(x, lrow, tid);
      // the next pass writes LDS again (every pass but a register-resident last one)
      if constexpr (p + 1 < NP - 1 || LAST_TO_LDS) __syncthreads();
      PDSP_STAMP(10 + 4 * p);  // LDS read-back issued + barrier
    }
  });
}

}  // namespace pdsp

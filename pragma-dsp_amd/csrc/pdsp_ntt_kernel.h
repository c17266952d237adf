// pdsp_ntt_kernel.h -- the number-theoretic transform over GF(2^64 - 2^32 + 1) (pdsp_goldilocks.h) and the exact cyclic
// convolution built on it, in the shape of the Stockham rows of pdsp_fft_rows_kernel.h: one row of N = 2^LOG2N points per
// TP = N / E threads, E points in registers, an autosort exchange through one LDS row between passes.
//
// A pass of radix R on Ns-point sub-transforms (Ns the product of the radices before it) takes, for j < N / R,
//   v[t] = x[j + t N/R] w^(t (j mod Ns)),   w = omega_(Ns R),   V = DFT_R(v),   y[(j / Ns) Ns R + (j mod Ns) + t Ns] = V[t]
// and the passes' radices multiply to N, so the last pass writes natural order.  A thread takes j = tid + u TP,
// u < E / R: in every pass it holds the points tid + TP m, m < E -- its loads from global memory, its reads of the LDS
// row and its stores of the last pass are unit-stride across lanes, and every thread stores exactly the positions it
// loaded (which is why the exact in-place call is safe).  Radices: E, ..., E and one last pass of 2^(LOG2N mod log2 E)
// where that is not 1.  DFT_R runs as log2 R radix-2 stages in registers whose constants are powers of
// omega_64 = 2^39, i.e. shifts; the inter-pass factors w^(t k) = omega_N^(t k N / (Ns R)) come from the handle's table
// omega_N^j, j < N / 2 (omega_N^(j + N/2) = -omega_N^j); the inverse runs the same passes on the inverse roots and
// multiplies by N^-1 = 2^(192 - LOG2N) at the store.  Every value between operations is canonical.
//
// CONV splits the N-point cyclic product into the two N/2-point products of one decimation-in-frequency stage, which
// the point-wise product does not mix:
//   u0[n] = a[n] + a[n + N/2],   u1[n] = (a[n] - a[n + N/2]) omega_N^n,   n < N/2       (b alike)
//   S_h = NTT_{N/2}^-1 (unscaled) of NTT_{N/2}(u_h(a)) . NTT_{N/2}(u_h(b)),   h = 0, 1
//   c[n] = N^-1 (S0[n] + omega_N^-n S1[n]),   c[n + N/2] = N^-1 (S0[n] - omega_N^-n S1[n])
// so that a thread of a 16-point-per-thread row runs 8 values of a's and 8 of b's half side by side (two half rows of
// LDS, each inter-pass factor fetched once for both) and holds 8 of S0 while S1 is made: half the registers of the
// undivided form, which at N = 16384 (1024 threads, 128 VGPRs each) does not fit.  The N/2-point passes run on
// omega_N^2 from the same table.  a and b are read once per half (one loop body runs both halves); the second read
// comes from the cache.
//
// LDS: the row is padded by one value per 16 (index i at i + i / 16): a radix-16 first pass writes at a lane stride of
// 16 values = 32 dwords, which the 32-bank rule of 8-byte writes would serialise 16-fold; padded, the 16 lanes of a
// write group fall on 16 distinct bank pairs.  The reads (lane stride 1) lose one bank pair per 32 lanes.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pdsp_goldilocks.h"

namespace pdsp {

enum NttOp { NTT_FORWARD = 0, NTT_INVERSE = 1, NTT_CONV = 2 };

// The shape of one instantiation: E points of the N-point row per thread (CONV: 16 at every size, 8 of each half).
template <int LOG2N, int OP>
struct NttTraits {
  static constexpr int N = 1 << LOG2N;
  static constexpr int LOG2E = OP == NTT_CONV || LOG2N >= 11 ? 4 : 3;
  static constexpr int E = 1 << LOG2E;
  static constexpr int TP = N / E;                     // threads of a row
  static constexpr int ROWS = TP >= 64 ? 1 : 64 / TP;  // rows of a workgroup: a whole wave at least
  static constexpr int WG = TP * ROWS;
  static constexpr int ROW_VALUES = N + N / 16;  // the padded LDS row (CONV: the two halves' rows)
  static constexpr size_t LDS_BYTES = (size_t)ROWS * ROW_VALUES * sizeof(uint64_t);
};

__device__ __forceinline__ constexpr int ntt_pad(int i) { return i + (i >> 4); }

constexpr int ntt_bitrev(int i, int bits) {
  int r = 0;
  for (int b = 0; b < bits; ++b) r |= ((i >> b) & 1) << (bits - 1 - b);
  return r;
}

// v <- DFT_R(v) on the roots omega_R = 2^(39 * 64 / R) (INV: their inverses), natural order in and out
template <int LOG2R, bool INV>
__device__ __forceinline__ void ntt_butterfly(uint64_t (&v)[1 << LOG2R]) {
  constexpr int R = 1 << LOG2R;
#pragma unroll
  for (int lg = LOG2R; lg >= 1; --lg) {
    const int len = 1 << lg, half = len >> 1;
#pragma unroll
    for (int b = 0; b < R; b += len) {
#pragma unroll
      for (int i = 0; i < half; ++i) {
        const uint64_t a = v[b + i], c = v[b + i + half];
        const int fs = (39 * i * (64 >> lg)) % 192;
        const int s = INV ? (192 - fs) % 192 : fs;
        v[b + i] = gl::add(a, c);
        v[b + i + half] = gl::mul_pow2(gl::sub(a, c), s);
      }
    }
  }
  uint64_t w[R];
#pragma unroll
  for (int i = 0; i < R; ++i) w[ntt_bitrev(i, LOG2R)] = v[i];
#pragma unroll
  for (int i = 0; i < R; ++i) v[i] = w[i];
}

// One row of `len` values in global memory, as a thread reads or writes it: value i taken mod p, zero at i >= len; a
// store at i >= len is dropped.  ONE (one row per workgroup, every size whose registers are scarce): the row is a buffer
// resource of len values -- the hardware's range check is the i < len, and an access costs one 32-bit offset register,
// where sixteen 64-bit addresses, clamps and predicates per row, hoisted and kept, spilled the 16384-point CONV.  The
// whole offset is the VGPR's, which the range check covers (a scalar offset is outside it).  Otherwise (several rows per
// workgroup, small N): plain pointers; every load is issued, none behind a branch, from an index clamped into the row.
typedef unsigned int ntt_u32x2 __attribute__((ext_vector_type(2)));
template <bool ONE>
struct NttRow {
  const uint64_t *p;
  int len;
  bool active;
  __amdgpu_buffer_rsrc_t rsrc;
  __device__ __forceinline__ NttRow(const uint64_t *base, int n, bool on) : p(base), len(n), active(on) {
    if constexpr (ONE) rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)base, 0, n * 8, 0x00020000);  // raw, 32-bit data
  }
  __device__ __forceinline__ uint64_t load(int i) const {
    if constexpr (ONE) {
      const ntt_u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, i * 8, 0, 0);
      return gl::canon(((uint64_t)v.y << 32) | v.x);
    } else {
      const unsigned j = (unsigned)i < (unsigned)(len - 1) ? (unsigned)i : (unsigned)(len - 1);  // len >= 1
      const uint64_t v = p[j];
      return active && i < len ? gl::canon(v) : 0;
    }
  }
  __device__ __forceinline__ void store(int i, uint64_t x) const {
    if constexpr (ONE) {
      const ntt_u32x2 v = {(unsigned)x, (unsigned)(x >> 32)};
      __builtin_amdgcn_raw_buffer_store_b64(v, rsrc, i * 8, 0, 0);
    } else {
      if (active && i < len) const_cast<uint64_t *>(p)[i] = x;
    }
  }
};

// omega_N^e (INV: omega_N^-e), 0 <= e < N = 2^LOG2N, from the table omega_N^j, j < N / 2 (a row of N / 2 values)
template <int LOG2N, bool INV, class Table>
__device__ __forceinline__ uint64_t ntt_root_power(const Table &tw, int e) {
  constexpr int N = 1 << LOG2N;
  const int idx = INV ? (N - e) & (N - 1) : e;
  const uint64_t w = tw.load(idx & (N / 2 - 1));
  return idx >= N / 2 ? gl::kP - w : w;  // no root is 0
}

// Passes PASS ... of NV transforms of 2^LOG2T points side by side (each factor omega^(t k) is fetched once for all of
// them), 2^LOG2E points per thread, on the table of omega_(2^LOG2W), LOG2W >= LOG2T (POW: below).  reg[v][m] = point
// tid + TP m of transform v on entry and on return; transform v exchanges through the padded LDS row at row + v ROW.
template <int LOG2T, int LOG2E, int LOG2W, bool INV, int NV, int ROW, bool POW, int PASS, class Table>
__device__ __forceinline__ void ntt_passes(uint64_t (&reg)[NV][1 << LOG2E], uint64_t *row, const Table &tw, int tid) {
  constexpr int N = 1 << LOG2T, E = 1 << LOG2E, TP = N / E;
  constexpr int LOG2NS = PASS * LOG2E, NS = 1 << LOG2NS;
  constexpr int LEFT = LOG2T - LOG2NS;
  constexpr int LOG2R = LEFT < LOG2E ? LEFT : LOG2E, R = 1 << LOG2R;
  constexpr bool LAST = LEFT <= LOG2E;
  constexpr int U = E / R;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int j = tid + u * TP, k = j & (NS - 1);
    const int j0 = ((j >> LOG2NS) << (LOG2NS + LOG2R)) + k;
    // pad(j0 + t NS) = pad(j0) + pad(t NS), one register and constants: NS is 1 (j0 a multiple of R, t < R <= 16), 8
    // (j0 mod 16 = k < 8, t NS mod 16 in {0, 8}) or a multiple of 16 -- the low four bits never carry
    static_assert(NS == 1 || NS == 8 || NS % 16 == 0, "the pad of a sum is the sum of the pads");
    const int wbase = ntt_pad(j0);
    uint64_t w[R];
    if constexpr (PASS > 0) {
      constexpr int STEP = (N / (NS * R)) << (LOG2W - LOG2T);
      if constexpr (!POW) {
#pragma unroll
        for (int t = 1; t < R; ++t) w[t] = ntt_root_power<LOG2W, INV>(tw, t * k * STEP);
      } else {  // CONV, short of registers: one fetch and R - 2 products, not R - 1 offsets that outlive the pass
        w[1] = ntt_root_power<LOG2W, INV>(tw, k * STEP);
#pragma unroll
        for (int t = 2; t < R; ++t) w[t] = gl::mul(w[t / 2], w[t - t / 2]);
      }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      uint64_t v[R];
#pragma unroll
      for (int t = 0; t < R; ++t) v[t] = PASS > 0 && t > 0 ? gl::mul(reg[i][u + t * U], w[t]) : reg[i][u + t * U];
      ntt_butterfly<LOG2R, INV>(v);
#pragma unroll
      for (int t = 0; t < R; ++t) {
        if constexpr (LAST)
          reg[i][u + t * U] = v[t];
        else
          row[i * ROW + wbase + ntt_pad(t * NS)] = v[t];
      }
    }
  }
  if constexpr (!LAST) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
      for (int m = 0; m < E; ++m)
        reg[i][m] = row[i * ROW + (TP % 16 == 0 ? ntt_pad(tid) + ntt_pad(TP * m) : ntt_pad(tid + TP * m))];
    __syncthreads();  // the next pass writes the rows these reads came from
    ntt_passes<LOG2T, LOG2E, LOG2W, INV, NV, ROW, POW, PASS + 1>(reg, row, tw, tid);
  }
}

// S_h of the rows ra and rb (CONV, above), unscaled: u_h of both rows (h = 0 the sums, h = 1 the differences times
// omega_N^n, n = tid + TP m, m < 8), their N/2-point transforms side by side, the product and its unscaled inverse
// transform, left in xy[0]
template <int LOG2N, class Row>
__device__ __forceinline__ void ntt_conv_half(uint64_t (&xy)[2][8], int h, const Row &ra, const Row &rb, uint64_t *row,
                                              const Row &tw, int tid) {
  using TR = NttTraits<LOG2N, NTT_CONV>;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int n = tid + TR::TP * m;
    const uint64_t a0 = ra.load(n), a1 = ra.load(n + TR::N / 2), b0 = rb.load(n), b1 = rb.load(n + TR::N / 2);
    if (h == 0) {
      xy[0][m] = gl::add(a0, a1), xy[1][m] = gl::add(b0, b1);
    } else {
      const uint64_t w = tw.load(n);
      xy[0][m] = gl::mul(gl::sub(a0, a1), w), xy[1][m] = gl::mul(gl::sub(b0, b1), w);
    }
  }
  ntt_passes<LOG2N - 1, 3, LOG2N, false, 2, TR::ROW_VALUES / 2, true, 0>(xy, row, tw, tid);
  uint64_t(&x)[1][8] = reinterpret_cast<uint64_t(&)[1][8]>(xy);
#pragma unroll
  for (int m = 0; m < 8; ++m) x[0][m] = gl::mul(xy[0][m], xy[1][m]);
  ntt_passes<LOG2N - 1, 3, LOG2N, true, 1, 0, true, 0>(x, row, tw, tid);
}

// One row per TP threads, ROWS rows per workgroup.  FORWARD / INVERSE: out = NTT(a) / NTT^-1(a), a_len = out_len = N.
// CONV: out[i] = sum_{j + l = i mod N} a[j] b[l], i < out_len; rows of a_len / b_len values, zero beyond;
// b_stride == 0 shares one b row.
template <int LOG2N, int OP>
__global__ __launch_bounds__((NttTraits<LOG2N, OP>::WG)) void ntt_kernel(
    const uint64_t *a, long long a_stride, int a_len, const uint64_t *b, long long b_stride, int b_len, uint64_t *out,
    long long out_stride, int out_len, const uint64_t *table, long long batch) {
  using TR = NttTraits<LOG2N, OP>;
  constexpr bool ONE = TR::ROWS == 1;
  extern __shared__ uint64_t ntt_lds[];
  const int sub = ONE ? 0 : (int)threadIdx.x / TR::TP;
  const int tid = ONE ? (int)threadIdx.x : (int)threadIdx.x % TR::TP;
  const long long r = (long long)blockIdx.x * TR::ROWS + sub;
  const bool active = r < batch;  // idle rows of the last workgroup run on zeros: the barriers want every thread
  uint64_t *const row = ntt_lds + (size_t)sub * TR::ROW_VALUES;
  const NttRow<ONE> ra(a + (active ? r : 0) * a_stride, a_len, active);
  const NttRow<ONE> ro(out + (active ? r : 0) * out_stride, out_len, active);
  const NttRow<ONE> tw(table, TR::N / 2, true);
  constexpr int SCALE = 192 - LOG2N;  // N^-1 = 2^SCALE
  if constexpr (OP == NTT_CONV) {
    static_assert(TR::E == 16, "CONV holds 8 values of each half per thread");
    const NttRow<ONE> rb(b + (active ? r : 0) * b_stride, b_len, active);
    uint64_t s0[8], xy[2][8];
#pragma unroll 1
    for (int h = 0; h < 2; ++h) {  // one body for both halves: half the code
      ntt_conv_half<LOG2N>(xy, h, ra, rb, row, tw, tid);
      if (h == 0) {
#pragma unroll
        for (int m = 0; m < 8; ++m) s0[m] = xy[0][m];
      }
    }
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int n = tid + TR::TP * m;
      const uint64_t c1 = gl::mul(xy[0][m], ntt_root_power<LOG2N, true>(tw, n));
      ro.store(n, gl::mul_pow2(gl::add(s0[m], c1), SCALE));
      ro.store(n + TR::N / 2, gl::mul_pow2(gl::sub(s0[m], c1), SCALE));
    }
  } else {
    uint64_t xs[1][TR::E];
    uint64_t(&x)[TR::E] = xs[0];
#pragma unroll
    for (int m = 0; m < TR::E; ++m) x[m] = ra.load(tid + TR::TP * m);
    ntt_passes<LOG2N, TR::LOG2E, LOG2N, OP == NTT_INVERSE, 1, 0, false, 0>(xs, row, tw, tid);
#pragma unroll
    for (int m = 0; m < TR::E; ++m)
      ro.store(tid + TR::TP * m, OP == NTT_FORWARD ? x[m] : gl::mul_pow2(x[m], SCALE));
  }
}

// out[i] = a[i] b[i] mod p, any 64-bit patterns in, canonical out
__global__ __launch_bounds__(256) void ntt_mul_kernel(const uint64_t *a, const uint64_t *b, uint64_t *out,
                                                      long long count) {
  const long long step = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += step)
    out[i] = gl::mul(gl::canon(a[i]), gl::canon(b[i]));
}

}  // namespace pdsp

// pdsp_packed.h -- the packed-real row that the FIR, STFT and DCT kernels share: a real row x of N = 2M points as the
// M-point complex row z[m] = x[2m] + i x[2m+1], transformed by TP = M/16 threads of E = 16 points each, the thread
// tid owning the pairs (k, M-k), k = tid + TP q.
//
// Forward split (PackedRow::forward_split).  With Z = FFT_M(z) and W = W_N^k, the N-point spectrum X of x is
//   S = Z[k] + conj Z[M-k],  P = W (Z[k] - conj Z[M-k]),  2 X[k] = S - iP,  2 X[M-k] = conj(S + iP)
// (S/2 and P/(2i) are the spectra of the even and the odd samples at k: X[k] = E + W O, X[M-k] = conj(E - W O)).
// Z[M] == Z[0]: the pair k = 0 gives X[0] and the Nyquist bin X[M]; k = M/2 pairs with itself.
//
// Inverse split (PackedRow::inverse_split), the same algebra backwards.  For a real row y with spectrum Y,
//   A = Y[k] + conj Y[M-k],  B = Y[k] - conj Y[M-k],  2 Z_y[k] = A + i W^-1 B,  2 Z_y[M-k] = conj(A) + i W conj(B)
// where Z_y = FFT_M(y[2m] + i y[2m+1]).  The split stores conj(2 Z_y) into the pair's own two LDS slots (every slot
// has exactly one owner: no barrier between the reads and the writes).  Fed Y / N, one set of FORWARD passes on those
// slots (PackedRow::second_transform) gives conj(y[2m] + i y[2m+1]) in registers: IFFT_M = conj FFT_M conj / M, and
// the 2 of the split and the 1/M of the inverse make the 1/N.
#pragma once

#include "pdsp_fft_core.h"

namespace pdsp {

// One row (or work item) of a packed-real kernel and this thread's part of it.  The kernel declares the LDS,
// __shared__ cx<T> lds[PackedRow<T, LOG2M>::TR::LDS_ELEMS], and passes the number of rows of the launch.
template <typename T, int LOG2M>
struct PackedRow {
  // sixteen points per thread, so that W_N^(TP q) = W_32^q.  (Eight at LOG2M = 13 -- half the registers, 8 waves per
  // SIMD, one more LDS pass -- measured 6 % slower on the spectrum kernel, tools/kbench; that option is gone.)
  static constexpr int LOG2E = 4;
  using TR = FftTraits<LOG2M, LOG2E>;
  static constexpr int E = TR::E, TP = TR::TP, M = TR::N;
  static_assert(LOG2M >= 5, "packed path: TP >= 2");

  int tid;
  bool live;
  long long row;  // this thread's row, clamped: dead rows of the last workgroup recompute the last live one
  cx<T> *lrow;    // the row's LDS slice, LROW >= M complex values

  // dead rows skip the stores but reach every barrier (count < 2^31 is checked on the host)
  __device__ __forceinline__ PackedRow(cx<T> *lds, const long long count) {
    tid = (int)(threadIdx.x % TP);
    const int rloc = (int)(threadIdx.x / TP);
    const long long raw = (long long)blockIdx.x * TR::ROWS + rloc;
    live = raw < count;
    row = uniform_row<TP>(live ? raw : count - 1);
    lrow = lds + rloc * TR::LROW;
  }

  // f(q, k) for the pairs k = tid + TP q, q < E/2 (k < M/2), and k = M/2, one more pair for tid == 0 (it pairs with
  // itself); q is an integral_constant
  template <class F>
  __device__ __forceinline__ void for_each_pair(F &&f) const {
    static_for<E / 2 + 1>([&](auto qc) {
      constexpr int q = qc;
      if (q < E / 2 || tid == 0) f(qc, tid + TP * q);
    });
  }

  // The forward split of the pair (k, M-k), k2 = (M - k) & (M - 1) (k = 0: Z[M] == Z[0]): Z[k] and Z[M-k] are read
  // from the row's LDS here, 2 X[k] = x(w) and 2 X[M-k] = xm(w), w = W_N^k, are formed where the kernel uses them
  // (its own loads for the pair go between the two)
  struct Split {
    cx<T> z, zp;
    __device__ __forceinline__ cx<T> s() const { return z + conj(zp); }
    __device__ __forceinline__ cx<T> p(const cx<T> w) const { return cmul(z - conj(zp), w); }
    __device__ __forceinline__ cx<T> x(const cx<T> w) const { return add_mul_neg_i(s(), p(w)); }
    __device__ __forceinline__ cx<T> xm(const cx<T> w) const { return conj(add_mul_pos_i(s(), p(w))); }
  };
  __device__ __forceinline__ Split forward_split(const int k, const int k2) const {
    return Split{lrow[lds_pad(k)], lrow[lds_pad(k2)]};
  }
  // The same for k = tid + TP q, at constant offsets from three bases made once behind the passes when TP % 16 == 0
  // (k, k2 then only name the pair): Z[k] at pad(tid) + cpad(TP q), Z[M-k] at pad(M - tid) - cpad(TP q), Z[M] == Z[0].
  // The six later families keep forward_split(k, k2): moving them changes their instruction streams; out of scope here.
  struct Pairs {
    const cx<T> *lrow, *zlo, *zhi, *zhi0;
    template <int q>
    __device__ __forceinline__ Split forward_split(std::integral_constant<int, q>, const int k, const int k2) const {
      if constexpr (TP % 16 == 0) return Split{zlo[cpad(TP * q)], q == 0 ? zhi0[0] : *(zhi - cpad(TP * q))};
      else return Split{lrow[lds_pad(k)], lrow[lds_pad(k2)]};
    }
  };
  __device__ __forceinline__ Pairs pairs(const cx<T> *const lrow) const {  // lrow: this row, as the kernel spells it
    return Pairs{lrow, lrow + lds_pad(tid), lrow + lds_pad(M - tid), lrow + lds_pad((M - tid) & (M - 1))};
  }

  // conj(2 Z_y[k]) and conj(2 Z_y[M-k]) into the row's LDS from ya = Y[k], yb = Y[M-k]; k2 = M - k, or that mod M
  // (read only when k != 0); w = W_N^k
  __device__ __forceinline__ void inverse_split(const int k, const int k2, const cx<T> ya, const cx<T> yb,
                                                const cx<T> w) const {
    const cx<T> a = ya + conj(yb), c = cmul(ya - conj(yb), conj(w));  // A, W_N^-k B
    lrow[lds_pad(k)] = conj(add_mul_pos_i(a, c));
    if (k != 0 && k2 != k) lrow[lds_pad(k2)] = add_mul_neg_i(a, c);
  }

  // after inverse_split: conj(y[2m] + i y[2m+1]) in slot q of x, m = tid + TP q
  template <class TWF>
  __device__ __forceinline__ void second_transform(cx<T> (&x)[E], const TWF &twf) const {
    __syncthreads();
    fft_pass_readback<T, LOG2M, LOG2E>(x, lrow, tid);
    __syncthreads();  // the first pass writes LDS again
    fft_passes<T, LOG2M, false, LOG2E>(x, lrow, twf, tid);
  }
};

// The twiddles of a packed-real row: the M-point transform's (twf: per-thread register bases when REG, by default
// when TP >= 16, else the table; spectrum_staged_kernel keeps register bases below that, its bits depend on it) and
// the split's, W_N^tid.  Where each kernel loads them is its own choice (load_order_fence's header).
template <typename T, int LOG2M, bool REG = (PackedRow<T, LOG2M>::TP >= 16)>
struct PackedTwiddles {
  using PR = PackedRow<T, LOG2M>;
  using V2 = typename vec2<T>::type;
  std::conditional_t<REG, RegTwiddles<T, LOG2M, PR::LOG2E>, TableTwiddles<T, LOG2M, PR::LOG2E>> twf;
  cx<T> twk0;

  __device__ __forceinline__ void load_passes(const V2 *tw, const int tid) {
    if constexpr (REG) twf.load(reinterpret_cast<const cx<T> *>(tw), tid);
    else twf.tw = reinterpret_cast<const cx<T> *>(tw);
  }
  __device__ __forceinline__ void load_split(const V2 *twr, const int tid) {
    twk0 = reinterpret_cast<const cx<T> *>(twr)[(unsigned)tid];
  }
  // the transform's tables, then the split's
  __device__ __forceinline__ void load(const V2 *tw, const V2 *twr, const int tid) {
    load_passes(tw, tid);
    load_split(twr, tid);
  }
  // W_N^k of pair q, k = tid + TP q: W_N^(TP q) = W_32^q
  template <int q>
  __device__ __forceinline__ cx<T> wk(std::integral_constant<int, q>) const {
    return mul_w32<T, q>(twk0);
  }
};

}  // namespace pdsp

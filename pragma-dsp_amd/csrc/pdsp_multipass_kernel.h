// pdsp_multipass_kernel.h -- transforms beyond the single-pass LDS limit: four-step passes, tile passes, transposing copy.
#pragma once

#include "pdsp_fft_core.h"

namespace pdsp {

// ---- four-step path for N beyond the single-pass LDS limit --------------------
// N = N1 * N2 with N2 = the largest single-pass size and 2 <= N1 <= 16.  Input index
// n = n1*N2 + n2, output index k = k1 + N1*k2.
//   A  (this kernel)  for every column n2: the N1-point DFT over n1 (stride N2), times
//      W_N^{n2*k1}, written back in the same [k1][n2] layout.  One thread per column, so
//      both its loads and stores are unit-stride across the lanes.
//   B  fft_stockham_kernel on the N1 rows of N2 points, in place.
//   C  (fourstep_out_kernel) transposes [k1][k2] -> k1 + N1*k2 with the 1/N of the inverse,
//      or reduces to amplitude / phase rows for the spectrum path.
// W_N^m = twa[m >> 9] * twb[m & 511]: two small host-built f64 tables, one product.
template <typename T, int LOG2N1, bool REAL_IN, bool HAS_WIN>
__global__ void __launch_bounds__(256)
fourstep_cols_kernel(const T *__restrict__ re, const T *__restrict__ im, const T *__restrict__ win,
                     T *__restrict__ sre, T *__restrict__ sim, const cx<T> *__restrict__ twa,
                     const cx<T> *__restrict__ twb, int n2, long long in_stride, long long frame_len,
                     long long batch) {
  constexpr int N1 = 1 << LOG2N1;
  const int cblocks = n2 / 256;
  const long long b = blockIdx.x / cblocks;
  const int col = (int)(blockIdx.x % cblocks) * 256 + (int)threadIdx.x;
  if (b >= batch) return;
  const size_t n = (size_t)N1 * (size_t)n2;
  const T *const xr = re + (size_t)b * (size_t)in_stride;
  const T *const xi = REAL_IN ? nullptr : im + (size_t)b * (size_t)in_stride;
  const long long last = frame_len - 1;  // REAL_IN rows may be shorter than N (buildFrame zero-padding)
  cx<T> a[N1];
  static_for<N1>([&](auto q) {
    const long long i = (long long)q * n2 + col;
    if constexpr (REAL_IN) {
      T v = ld_stream(xr + (size_t)(i < last ? i : last));
      v = i <= last ? v : T(0);
      if constexpr (HAS_WIN) v *= win[i];
      a[q] = cx<T>{v, T(0)};
    } else {
      a[q] = cx<T>{ld_stream(xr + (size_t)i), ld_stream(xi + (size_t)i)};
    }
  });
  fft_reg<T, N1>(a);
  T *const orow = sre + (size_t)b * n, *const irow = sim + (size_t)b * n;
  static_for<N1>([&](auto k1) {
    cx<T> v = a[bitrev(k1, LOG2N1)];
    if constexpr (k1 > 0) {
      const unsigned m = (unsigned)col * (unsigned)k1;  // < N <= 2^18
      v = cmul(v, cmul(twa[m >> 9], twb[m & 511]));
    }
    orow[(size_t)k1 * n2 + col] = v.x;
    irow[(size_t)k1 * n2 + col] = v.y;
  });
}

// Pass C.  MODE 0: complex planes out (times `scale`); MODE 1: amplitude (+ phase) rows of
// spectrum(), bins = N/2+1 or N.  One thread per k2, N1 consecutive outputs each.
template <typename T, int LOG2N1, int MODE>
__global__ void __launch_bounds__(256)
fourstep_out_kernel(const T *__restrict__ sre, const T *__restrict__ sim, T *__restrict__ ore, T *__restrict__ oim,
                    int n2, T scale, int bins, int nyq, T s_edge, T s_mid, long long batch) {
  constexpr int N1 = 1 << LOG2N1;
  const int cblocks = n2 / 256;
  const long long b = blockIdx.x / cblocks;
  const int k2 = (int)(blockIdx.x % cblocks) * 256 + (int)threadIdx.x;
  if (b >= batch) return;
  const size_t n = (size_t)N1 * (size_t)n2;
  const T *const rr = sre + (size_t)b * n, *const ri = sim + (size_t)b * n;
  T vr[N1], vi[N1];
  static_for<N1>([&](auto k1) {
    vr[k1] = rr[(size_t)k1 * n2 + k2];
    vi[k1] = ri[(size_t)k1 * n2 + k2];
  });
  if constexpr (MODE == 0) {
    T *const o1 = ore + (size_t)b * n + (size_t)k2 * N1, *const o2 = oim + (size_t)b * n + (size_t)k2 * N1;
    static_for<N1>([&](auto k1) {
      o1[k1] = vr[k1] * scale;
      o2[k1] = vi[k1] * scale;
    });
  } else {
    T *const arow = ore + (size_t)b * (size_t)bins, *const prow = oim ? oim + (size_t)b * (size_t)bins : nullptr;
    static_for<N1>([&](auto k1) {
      const int k = k2 * N1 + k1;
      if (k < bins) {
        arow[k] = mag(cx<T>{vr[k1], vi[k1]}) * ((k == 0 || k == nyq) ? s_edge : s_mid);
        if (prow) prow[k] = T(atan2(vi[k1], vr[k1]));
      }
    });
  }
}

// ---- tile passes: two passes for 2^15 <= N <= 2^18, three for 2^19 <= N <= 2^27 (f32) -----------
// N is cut into BALANCED factors of 64 ... 512 points instead of N1 * 16384, and every pass is one launch
// of tile_pass_kernel: a 256-thread workgroup owns TILE transforms of one factor, moves them between HBM
// and LDS in 128 ... 256-byte segments, runs them in LDS (fft_passes on the tile's LDS rows, 256/TP rows
// per round), and writes them back -- the transposition that a multi-pass transform needs happens in LDS.
//
// Two passes, N = A*B: n = n1*B + n2, k = k1 + A*k2,
//   X[k1 + A k2] = sum_n2 W_B^(n2 k2) * [ W_N^(n2 k1) * sum_n1 x[n1 B + n2] W_A^(n1 k1) ].
//   pass 1 (COLS): A-point transforms down the columns n2, times W_N^(n2 k1), written back in place of
//                  the matrix [k1][n2];
//   pass 2 (ROWS): B-point transforms along the rows k1, written TRANSPOSED to k1 + A*k2.
// Three passes, N = A*B*C: n = (n1*B + n2)*C + n3, k = k1 + A*(k2 + B*k3); with n' = n2*C + n3,
//   W_N^(n k) = W_A^(n1 k1) * W_N^(n' k1) * W_B^(n2 k2) * W_BC^(n3 k2) * W_C^(n3 k3):
//   pass 1 (COLS): A-point transforms over n1 (stride B*C) for every column n', times W_N^(n' k1), in place;
//   pass 2 (COLS): for every k1, B-point transforms over n2 (stride C) for every n3, times
//                  W_BC^(n3 k2) = W_N^(A n3 k2), written to row k2*A + k1 (so that pass 3 finds rows of
//                  consecutive k1 next to each other);
//   pass 3 (ROWS): C-point transforms along the rows, written transposed to (k2*A + k1) + A*B*k3.
// HBM traffic is 16 B per sample per pass (32 / 48 B for 16 algorithmic) where round 1's forms made three
// passes (N1 <= 16 columns / 16384-point rows / transposing copy) up to 2^18 and five above.
//
// Geometry of one launch (TileGeom): blockIdx -> (batch row b, block blk < nblk, tile < tiles);
//   COLS: element (p, j), p < L, j < TILE:  in[b*N + blk*in_blk + tile*TILE + p*in_stride + j]
//                                          out[b*N + blk*out_blk + tile*TILE + p*out_stride + j]
//         times W_N^(tmul * (tile*TILE + j) * p);
//   ROWS: TILE whole rows of L contiguous points from in[b*N + tile*TILE*L]; row i, output p goes to
//         out[b*N + tile*TILE + i + p*out_stride], times `scale`.
// LDS rows are LROWX = LROW + (2 - LROW) mod 8 elements apart: a lane quad writes one element to each of
// four rows, and four rows of LROW (a multiple of 8 for L >= 128) would land on the same banks.
//   tw = radix table of the L-point transform; W_N^m = twa[m >> 9] * twb[m & 511].
struct TileGeom {
  long long n;          // N: distance between batch rows on the output side (and on the input side unless in_batch)
  int nblk, tiles;      // blocks per transform, tiles per block
  long long in_blk, out_blk, in_stride, out_stride;
  unsigned tmul;        // twiddle exponent multiplier (1, or A in the middle pass of three)
  long long in_batch;   // distance between batch rows of the input (frames of spectrum(): the caller's stride,
                        // in real samples)
  unsigned tshift;      // 0, or 1 when twa / twb belong to a plan of 2N points (W_N^m = W_2N^(2m): the
                        // N/2-point transform of the packed-real spectrum path on its N-point plan's tables)
  // IN = 5 / 6: createWindow fused into the packed first pass (cosine-sum windows, fourier.ts:14-52, evaluated by
  // angle addition instead of being read back, 4 bytes per sample): with f = 2 pi / (frame length - 1) and
  // cs(t) = (cos t, sin t), sample n = 8 u + 2 in_stride SPI ic + e has
  //   cs(f n) = wa[u >> 9] * wb[u & 511] * wstep[ic] * we[e]     (wa[i] = cs(4096 f i), wb[j] = cs(8 f j),
  //   wstep[ic] = cs(2 f in_stride SPI ic), we[e] = cs(f e); all built in f64 on the host)
  // and w = k0 + k1 c (IN = 5) or k0 + c (k1 + k2 c) (IN = 6), c = cos(f n).
  const float *wa, *wb, *wstep, *we;
  float k0, k1, k2;
  // Scratch planes between the first two of three passes, TILE-MAJOR (0 = natural order everywhere): a strided
  // tile costs its READER (the column passes run at 4.9-5.7 TB/s, the row passes -- contiguous reads, strided
  // writes -- at 6.1-6.3), so the first pass writes column n' = n2 C + n3 of every row block to
  //   ((n3 >> perm_lt) * perm_b + n2) << perm_lt | (n3 & (2^perm_lt - 1))       (perm_lc = log2 C, perm_b = B)
  // i.e. the [B][2^perm_lt] tile the second pass needs becomes one contiguous chunk (in_tile = B << perm_lt apart,
  // in_stride = 2^perm_lt), and the first pass still writes segments of the same width at the same stride.
  int perm_lc, perm_lt, perm_b;  // output side; perm_lt == 0: no permutation
  long long in_tile;            // input side: distance between the origins of consecutive tiles (0: TILE)
};

// IN (first pass only; in_im then carries the window table or nothing):
//   0  complex planes
//   1  real rows: the first pass of Radix2Fft.forward / spectrum(), no imaginary plane
//   2  real rows times the window table (applyWindow on load, window value at the sample's index in the frame)
//   3  PACKED real rows: point m of the N-point transform is (x[2m], x[2m+1]) of a 2N-sample frame -- the
//      packed-real form of spectrum() (split_amp_rows_kernel undoes the packing)
//   4  packed real rows times the window table
//   5  packed real rows times a two-term cosine-sum window evaluated in registers (TileGeom::wa ...)
//   6  the same, three-term (blackman)
template <typename T, int LOG2L, int TILE, bool COLS, int IN = 0>
__global__ void __launch_bounds__(256)
tile_pass_kernel(const T *__restrict__ in_re, const T *__restrict__ in_im, T *__restrict__ out_re, T *__restrict__ out_im,
                 const typename vec2<T>::type *__restrict__ tw, const cx<T> *__restrict__ twa,
                 const cx<T> *__restrict__ twb, const TileGeom g, const T scale, const long long batch) {
  static_assert(IN == 0 || COLS, "real / packed / windowed input rides on the first (column) pass");
  constexpr bool REAL_IN = IN == 1 || IN == 2, WINDOWED = IN == 2 || IN == 4, PACKED = IN >= 3, FUSEDWIN = IN >= 5;
  static_assert(!FUSEDWIN || sizeof(T) == 4, "fused windows: f32");
  using TR = FftTraits<LOG2L>;
  constexpr int L = TR::N, E = TR::E, TP = TR::TP, RPR = 256 / TP, ROUNDS = TILE / RPR;
  static_assert(LOG2L >= 6 && LOG2L <= 9 && TILE % RPR == 0 && TILE % 4 == 0 && ROUNDS >= 1, "tile of whole rounds");
  constexpr int LROWX = TR::LROW + ((2 - TR::LROW % 8) + 8) % 8;
  constexpr int TS = TILE / 4, SPI = 256 / TS;  // threads per tile segment, segments per wave of accesses
  static_assert(L % SPI == 0, "whole accesses");
  typedef T V4 __attribute__((ext_vector_type(4)));
  __shared__ cx<T> lds[TILE * LROWX];

  const int t = (int)threadIdx.x;
  const long long per = (long long)g.nblk * g.tiles;
  const long long b = (long long)blockIdx.x / per;
  const int rem = (int)((long long)blockIdx.x % per);
  const int blk = rem / g.tiles, t0 = (rem % g.tiles) * TILE;
  if (b >= batch) return;
  const size_t base = (size_t)b * (size_t)g.n;
  const int seg = t / TS, j4 = (t % TS) * 4;

  // COLS: the inter-pass twiddles W_N^(tmul (t0 + j4 + j) p), p = seg + SPI ic.  Tables first (the lesson of
  // the single-pass kernels, load_order_fence's header): four two-level lookups per lane up here, their L2 latency
  // under the tile's HBM loads, and one product per iteration below -- instead of four gathers per iteration
  // between the transforms and the stores.  With q = tmul << tshift, J = t0 + j4:
  //   w(ic)  = W^(q p J) = W^(q seg J) * (W^(q SPI J))^ic          first element of the lane's four
  //   ws(ic) = W^(q p)   = W^(q seg)   * (W^(q SPI))^ic            step from element j to j + 1
  cx<T> tw_w{T(1), T(0)}, tw_wv{T(1), T(0)}, tw_s{T(1), T(0)}, tw_su{T(1), T(0)};
  if constexpr (COLS) {
    const unsigned q = g.tmul << g.tshift, J = (unsigned)(t0 + j4);
    const unsigned m0 = q * (unsigned)seg * J, mv = q * (unsigned)SPI * J;  // < N <= 2^27 (of the tables' plan)
    const unsigned s0 = q * (unsigned)seg, su = q * (unsigned)SPI;
    tw_w = cmul(twa[m0 >> 9], twb[m0 & 511]);
    tw_wv = cmul(twa[mv >> 9], twb[mv & 511]);
    tw_s = cmul(twa[s0 >> 9], twb[s0 & 511]);
    tw_su = cmul(twa[su >> 9], twb[su & 511]);
  }
  if constexpr (COLS) {
    // strided tile in: element (p, j) -> LDS row j, position p
    const size_t in_off = (size_t)blk * (size_t)g.in_blk +
                          (g.in_tile ? (size_t)(t0 / TILE) * (size_t)g.in_tile + (size_t)j4 : (size_t)(t0 + j4));  // index inside the frame
    const size_t ibase = (size_t)b * (size_t)g.in_batch + in_off;
    cx<T> wcs{T(1), T(0)};  // FUSEDWIN: cs(f n) of the lane's first sample at ic = 0
    if constexpr (FUSEDWIN) {
      const unsigned u = (unsigned)((in_off + (size_t)seg * (size_t)g.in_stride) >> 2);  // sample index / 8
      wcs = cmul(reinterpret_cast<const cx<T> *>(g.wa)[u >> 9], reinterpret_cast<const cx<T> *>(g.wb)[u & 511]);
    }
    static_for<L / SPI>([&](auto ic) {
      const int p = seg + SPI * ic;
      if constexpr (PACKED) {
        // four points = eight consecutive samples of the frame (32 bytes per lane, TILE * 8 per segment)
        const size_t fo = 2 * (in_off + (size_t)p * (size_t)g.in_stride);  // sample index inside the frame
        const T *const src = in_re + (size_t)b * (size_t)g.in_batch + fo;
        V4 r0 = ld_stream(reinterpret_cast<const V4 *>(src)), r1 = ld_stream(reinterpret_cast<const V4 *>(src) + 1);
        if constexpr (WINDOWED) {
          r0 = r0 * *reinterpret_cast<const V4 *>(in_im + fo);
          r1 = r1 * *(reinterpret_cast<const V4 *>(in_im + fo) + 1);
        }
        if constexpr (FUSEDWIN) {
          const cx<T> *const wst = reinterpret_cast<const cx<T> *>(g.wstep), *const wee = reinterpret_cast<const cx<T> *>(g.we);
          const cx<T> c0 = cmul(wcs, wst[ic]);  // wave-uniform step: scalar loads
          cx<T> w[4];
          fused_window_pairs<T, IN == 6>(c0, wee, g.k0, g.k1, g.k2, w);
          r0 = r0 * V4{w[0].x, w[0].y, w[1].x, w[1].y};
          r1 = r1 * V4{w[2].x, w[2].y, w[3].x, w[3].y};
        }
        cx<T> *const d = lds + j4 * LROWX + lds_pad(p);
        d[0 * LROWX] = cx<T>{r0.x, r0.y};
        d[1 * LROWX] = cx<T>{r0.z, r0.w};
        d[2 * LROWX] = cx<T>{r1.x, r1.y};
        d[3 * LROWX] = cx<T>{r1.z, r1.w};
        return;
      }
      const size_t gi = ibase + (size_t)p * (size_t)g.in_stride;
      V4 r = ld_stream(reinterpret_cast<const V4 *>(in_re + gi));
      V4 m = V4{T(0), T(0), T(0), T(0)};
      if constexpr (!REAL_IN) m = ld_stream(reinterpret_cast<const V4 *>(in_im + gi));
      // WINDOWED: in_im is the window table (N values), indexed like the frame
      if constexpr (WINDOWED) r = r * *reinterpret_cast<const V4 *>(in_im + in_off + (size_t)p * (size_t)g.in_stride);
      cx<T> *const d = lds + j4 * LROWX + lds_pad(p);
      d[0 * LROWX] = cx<T>{r.x, m.x};
      d[1 * LROWX] = cx<T>{r.y, m.y};
      d[2 * LROWX] = cx<T>{r.z, m.z};
      d[3 * LROWX] = cx<T>{r.w, m.w};
    });
  } else {
    // TILE whole rows, one contiguous chunk per plane
    const size_t cbase = base + (size_t)t0 * L;
    static_for<TILE * L / 4 / 256>([&](auto ic) {
      const int e = 4 * (t + 256 * ic);
      const V4 r = ld_stream(reinterpret_cast<const V4 *>(in_re + cbase + e));
      const V4 m = ld_stream(reinterpret_cast<const V4 *>(in_im + cbase + e));
      cx<T> *const d = lds + (e / L) * LROWX + lds_pad(e % L);  // 4 points never straddle a 16-block
      d[0] = cx<T>{r.x, m.x};
      d[1] = cx<T>{r.y, m.y};
      d[2] = cx<T>{r.z, m.z};
      d[3] = cx<T>{r.w, m.w};
    });
  }
  __syncthreads();

  const int tid = t % TP, rloc = t / TP;
  RegTwiddles<T, LOG2L> twf;
  twf.load(reinterpret_cast<const cx<T> *>(tw), tid);
  static_for<ROUNDS>([&](auto rc) {
    cx<T> *const lrow = lds + (rc * RPR + rloc) * LROWX;
    cx<T> x[E];
    static_for<E>([&](auto q) { x[q] = lrow[lds_pad(tid + TP * q)]; });
    __syncthreads();  // the first pass scatters into the same rows
    fft_passes<T, LOG2L, true>(x, lrow, twf, tid);  // natural order in LDS
  });
  __syncthreads();

  // strided tile out: element (p, j) -> out[... + p*out_stride + j]
  size_t ocol = (size_t)(t0 + j4);
  if constexpr (COLS) {
    if (g.perm_lt) {  // tile-major scratch (TileGeom): the lane's four columns stay adjacent (2^perm_lt >= 16)
      const unsigned np = (unsigned)(t0 + j4), n2 = np >> g.perm_lc, n3 = np & ((1u << g.perm_lc) - 1u);
      ocol = ((size_t)((n3 >> g.perm_lt) * (unsigned)g.perm_b + n2) << g.perm_lt) | (size_t)(n3 & ((1u << g.perm_lt) - 1u));
    }
  }
  const size_t obase = COLS ? base + (size_t)blk * (size_t)g.out_blk + ocol : base + ocol;
  static_for<L / SPI>([&](auto ic) {
    const int p = seg + SPI * ic;
    const cx<T> *const d = lds + j4 * LROWX + lds_pad(p);
    cx<T> v[4] = {d[0 * LROWX], d[1 * LROWX], d[2 * LROWX], d[3 * LROWX]};
    if constexpr (COLS) {
      // W_N^(tmul (t0 + j4 + j) p), j = 0..3: w(ic) for j = 0, then steps of ws(ic) (both advanced below)
      cx<T> w = tw_w;
      v[0] = cmul(v[0], w);
      static_for<3>([&](auto jc) {
        w = cmul(w, tw_s);
        v[jc + 1] = cmul(v[jc + 1], w);
      });
      if constexpr (ic + 1 < L / SPI) {
        tw_w = cmul(tw_w, tw_wv);
        tw_s = cmul(tw_s, tw_su);
      }
    } else {
      static_for<4>([&](auto jc) { v[jc] = v[jc] * scale; });
    }
    const size_t go = obase + (size_t)p * (size_t)g.out_stride;
    st_stream(V4{v[0].x, v[1].x, v[2].x, v[3].x}, reinterpret_cast<V4 *>(out_re + go));
    st_stream(V4{v[0].y, v[1].y, v[2].y, v[3].y}, reinterpret_cast<V4 *>(out_im + go));
  });
}

// tile_pass_kernel's COLS pass for a 512-point factor on tiles of 32 columns (plain tiles: 16 columns, 64-byte
// strided segments -- the width at which the memory system collapses, tools/kbench3).  One radix-2
// decimation-in-FREQUENCY step over two 256-point halves that the same 256 threads run back to back through the
// same 70 KB of LDS: a lane loads x[p] and x[p + 256] of its four columns, u[p] = x[p] + x[p + 256] goes to LDS,
// v[p] = (x[p] - x[p + 256]) W_512^p waits in 64 registers; FFT_256(u) = the even output rows k1 = 2k,
// FFT_256(v) = the odd ones k1 = 2k + 1.  Geometry (tiles = columns / 32), the tile-major scratch options and the
// inter-pass twiddles W_N^(tmul col k1) (hoisted two-level lookups) as tile_pass_kernel's COLS; IN = 0 complex
// planes, 1 real rows.  tw = radix table of the 256-point transform.
template <typename T, int IN>
__global__ void __launch_bounds__(256, 2)
tile_cols512_kernel(const T *__restrict__ in_re, const T *__restrict__ in_im, T *__restrict__ out_re, T *__restrict__ out_im,
                    const typename vec2<T>::type *__restrict__ tw, const cx<T> *__restrict__ twa,
                    const cx<T> *__restrict__ twb, const TileGeom g, const long long batch) {
  static_assert(IN == 0 || IN == 1, "complex planes or real rows");
  constexpr bool REAL_IN = IN == 1;
  using TR = FftTraits<8>;
  constexpr int TILE = 32, H = 256, E = TR::E, TP = TR::TP, RPR = 256 / TP, ROUNDS = TILE / RPR;
  constexpr int LROWX = TR::LROW + ((2 - TR::LROW % 8) + 8) % 8;
  constexpr int TS = TILE / 4, SPI = 256 / TS, NIT = H / SPI;  // 8 lanes per segment, 32 rows per access, 8 accesses
  typedef T V4 __attribute__((ext_vector_type(4)));
  __shared__ cx<T> lds[TILE * LROWX];

  const int t = (int)threadIdx.x;
  const long long per = (long long)g.nblk * g.tiles;
  const long long b = (long long)blockIdx.x / per;
  const int rem = (int)((long long)blockIdx.x % per);
  const int blk = rem / g.tiles, t0 = (rem % g.tiles) * TILE;
  if (b >= batch) return;
  const size_t base = (size_t)b * (size_t)g.n;
  const int seg = t / TS, j4 = (t % TS) * 4;
  const int tid = t % TP, rloc = t / TP;

  // tables first.  Output row k1 = 2 (seg + SPI ic) + o (o = 0: even half, 1: odd half); q = tmul << tshift, J = t0 + j4:
  //   first column of the lane's four: W^(q J k1) = W^(q J 2 seg) * (W^(q J 2 SPI))^ic   [* W^(q J) for o = 1]
  //   step to the next column:         W^(q k1)   = W^(q 2 seg)   * (W^(q 2 SPI))^ic     [* W^q     for o = 1]
  RegTwiddles<T, 8> twf;
  twf.load(reinterpret_cast<const cx<T> *>(tw), tid);
  const unsigned q = g.tmul << g.tshift, J = (unsigned)(t0 + j4);
  auto look = [&](unsigned m) { return cmul(twa[m >> 9], twb[m & 511]); };
  const cx<T> w_first0 = look(q * J * (unsigned)(2 * seg)), w_first_step = look(q * J * (unsigned)(2 * SPI));
  const cx<T> w_col0 = look(q * (unsigned)(2 * seg)), w_col_step = look(q * (unsigned)(2 * SPI));
  const cx<T> w_odd_first = look(q * J), w_odd_col = look(q);
  const cx<T> ws = look(((unsigned)(g.n >> 9) << g.tshift) * (unsigned)seg);  // W_512^seg; W_512^(seg + 32 ic) = ws W_16^ic
  cx<T> wv[NIT];
  static_for<NIT>([&](auto ic) {
    constexpr int i = ic;
    wv[i] = mul_w16<T, i>(ws);
  });

  // strided tile in: rows p and p + 256 of the lane's four columns; every load first
  const size_t in_off = (size_t)blk * (size_t)g.in_blk +
                        (g.in_tile ? (size_t)(t0 / TILE) * (size_t)g.in_tile + (size_t)j4 : (size_t)(t0 + j4));
  const size_t ibase = (size_t)b * (size_t)g.in_batch + in_off;
  V4 ra[NIT], ma[NIT], rb[NIT], mb[NIT];
  static_for<NIT>([&](auto ic) {
    const size_t gi = ibase + (size_t)(seg + SPI * ic) * (size_t)g.in_stride, gj = gi + (size_t)H * (size_t)g.in_stride;
    ra[ic] = ld_stream(reinterpret_cast<const V4 *>(in_re + gi));
    rb[ic] = ld_stream(reinterpret_cast<const V4 *>(in_re + gj));
    if constexpr (!REAL_IN) {
      ma[ic] = ld_stream(reinterpret_cast<const V4 *>(in_im + gi));
      mb[ic] = ld_stream(reinterpret_cast<const V4 *>(in_im + gj));
    }
  });
  cx<T> v[NIT][4];
  static_for<NIT>([&](auto ic) {
    const V4 z = V4{T(0), T(0), T(0), T(0)};
    const V4 r1 = ra[ic], r2 = rb[ic], m1 = REAL_IN ? z : ma[ic], m2 = REAL_IN ? z : mb[ic];
    const cx<T> a[4] = {cx<T>{r1.x, m1.x}, cx<T>{r1.y, m1.y}, cx<T>{r1.z, m1.z}, cx<T>{r1.w, m1.w}};
    const cx<T> c[4] = {cx<T>{r2.x, m2.x}, cx<T>{r2.y, m2.y}, cx<T>{r2.z, m2.z}, cx<T>{r2.w, m2.w}};
    cx<T> *const d = lds + j4 * LROWX + lds_pad(seg + SPI * ic);
    static_for<4>([&](auto jc) {
      v[ic][jc] = cmul(a[jc] - c[jc], wv[ic]);
      d[jc * LROWX] = a[jc] + c[jc];
    });
  });
  __syncthreads();

  size_t ocol = (size_t)(t0 + j4);
  if (g.perm_lt) {  // tile-major scratch (TileGeom)
    const unsigned np = (unsigned)(t0 + j4), n2 = np >> g.perm_lc, n3 = np & ((1u << g.perm_lc) - 1u);
    ocol = ((size_t)((n3 >> g.perm_lt) * (unsigned)g.perm_b + n2) << g.perm_lt) | (size_t)(n3 & ((1u << g.perm_lt) - 1u));
  }
  const size_t obase = base + (size_t)blk * (size_t)g.out_blk + ocol;
  static_for<2>([&](auto oc) {
    constexpr int o = oc;
    if constexpr (o == 1) {  // the odd half: v from the registers into the same rows
      __syncthreads();       // (the even half's tile has been read out)
      static_for<NIT>([&](auto ic) {
        cx<T> *const d = lds + j4 * LROWX + lds_pad(seg + SPI * ic);
        static_for<4>([&](auto jc) { d[jc * LROWX] = v[ic][jc]; });
      });
      __syncthreads();
    }
    static_for<ROUNDS>([&](auto rc) {
      cx<T> *const lrow = lds + (rc * RPR + rloc) * LROWX;
      cx<T> x[E];
      static_for<E>([&](auto qq) { x[qq] = lrow[lds_pad(tid + TP * qq)]; });
      __syncthreads();  // the first pass scatters into the same rows
      fft_passes<T, 8, true>(x, lrow, twf, tid);  // natural order in LDS
    });
    __syncthreads();
    // strided tile out: element (k, j) -> out[... + (2 k + o) * out_stride + j], times W_N^(tmul col k1)
    cx<T> tw_w = o == 1 ? cmul(w_first0, w_odd_first) : w_first0, tw_s = o == 1 ? cmul(w_col0, w_odd_col) : w_col0;
    static_for<NIT>([&](auto ic) {
      const int k1 = 2 * (seg + SPI * ic) + o;
      const cx<T> *const d = lds + j4 * LROWX + lds_pad(seg + SPI * ic);
      cx<T> y[4] = {d[0 * LROWX], d[1 * LROWX], d[2 * LROWX], d[3 * LROWX]};
      cx<T> w = tw_w;
      y[0] = cmul(y[0], w);
      static_for<3>([&](auto jc) {
        w = cmul(w, tw_s);
        y[jc + 1] = cmul(y[jc + 1], w);
      });
      if constexpr (ic + 1 < NIT) {
        tw_w = cmul(tw_w, w_first_step);
        tw_s = cmul(tw_s, w_col_step);
      }
      const size_t go = obase + (size_t)k1 * (size_t)g.out_stride;
      st_stream(V4{y[0].x, y[1].x, y[2].x, y[3].x}, reinterpret_cast<V4 *>(out_re + go));
      st_stream(V4{y[0].y, y[1].y, y[2].y, y[3].y}, reinterpret_cast<V4 *>(out_im + go));
    });
  });
}

// tile_pass_kernel's ROWS pass for a 512-point factor on tiles of 32 rows.  As a plain tile a 512-point factor
// fits 16 rows (70 KB of LDS), i.e. 64-byte output segments: 5.0 TB/s per pass, against 6.1 for the 32-row
// tiles of a 256-point factor (rocprofv3, profiles/r02_experiments/tile_pass_times_per_kernel.csv).  Here the
// factor is one radix-2 decimation-in-TIME step over two 256-point transforms that the same 256 threads run back
// to back through the same 70 KB (spectrum_dif16k_kernel's idea, the other way round): a lane's 16-byte loads
// bring x[p .. p+3] of a row, the even samples go to LDS, the odd ones wait in 64 registers;
//   E = FFT_256(x[2m]) is read back in OUTPUT layout (four rows per lane, 64 registers), O = FFT_256(x[2m+1])
//   follows through the same rows, and X[k] = E[k] + W_512^k O[k], X[k + 256] = E[k] - W_512^k O[k]
// leave as 128-byte segments (32 consecutive rows) at k and k + 256.  Geometry as tile_pass_kernel's ROWS
// (tiles = rows / 32); tw = radix table of the 256-point transform; W_512^k from the plan's two-level table.
template <typename T>
__global__ void __launch_bounds__(256, 2)
tile_rows512_kernel(const T *__restrict__ in_re, const T *__restrict__ in_im, T *__restrict__ out_re, T *__restrict__ out_im,
                    const typename vec2<T>::type *__restrict__ tw, const cx<T> *__restrict__ twa,
                    const cx<T> *__restrict__ twb, const TileGeom g, const T scale, const long long batch) {
  using TR = FftTraits<8>;
  constexpr int L = 512, H = 256, TILE = 32, E = TR::E, TP = TR::TP, RPR = 256 / TP, ROUNDS = TILE / RPR;
  constexpr int LROWX = TR::LROW + ((2 - TR::LROW % 8) + 8) % 8;
  constexpr int TS = TILE / 4, SPI = 256 / TS, NIN = TILE * L / 4 / 256, NOUT = H / SPI;  // 16 loads, 8 output rounds
  typedef T V4 __attribute__((ext_vector_type(4)));
  __shared__ cx<T> lds[TILE * LROWX];

  const int t = (int)threadIdx.x;
  const long long b = (long long)blockIdx.x / g.tiles;
  const int t0 = (int)((long long)blockIdx.x % g.tiles) * TILE;
  if (b >= batch) return;
  const size_t base = (size_t)b * (size_t)g.n;
  const int seg = t / TS, j4 = (t % TS) * 4;
  const int tid = t % TP, rloc = t / TP;

  // tables first: the 256-point transform's bases and W_512^seg (W_512^(seg + 32 ic) = W_512^seg * W_16^ic)
  RegTwiddles<T, 8> twf;
  twf.load(reinterpret_cast<const cx<T> *>(tw), tid);
  const unsigned m512 = ((unsigned)(g.n >> 9) << g.tshift) * (unsigned)seg;
  const cx<T> wseg = cmul(twa[m512 >> 9], twb[m512 & 511]);

  // TILE whole rows, one contiguous chunk per plane: lane t, load ic holds points p .. p+3 of row (t >> 7) + 2 ic,
  // p = 4 (t & 127): even samples 2m, 2m + 2 -> E's inputs m, m + 1 (m = 2 (t & 127)); odd samples -> O's
  const size_t cbase = base + (size_t)t0 * L;
  V4 r[NIN], mi[NIN];
  static_for<NIN>([&](auto ic) {
    const int e = 4 * (t + 256 * ic);
    r[ic] = ld_stream(reinterpret_cast<const V4 *>(in_re + cbase + e));
    mi[ic] = ld_stream(reinterpret_cast<const V4 *>(in_im + cbase + e));
  });
  const int me = 2 * (t & 127), lrow0 = t >> 7;
  cx<T> od[NIN][2];
  static_for<NIN>([&](auto ic) {
    cx<T> *const d = lds + (lrow0 + 2 * ic) * LROWX + lds_pad(me);  // me is even: me, me + 1 share a 16-block
    d[0] = cx<T>{r[ic].x, mi[ic].x};
    d[1] = cx<T>{r[ic].z, mi[ic].z};
    od[ic][0] = cx<T>{r[ic].y, mi[ic].y};
    od[ic][1] = cx<T>{r[ic].w, mi[ic].w};
  });
  __syncthreads();

  auto transform_rows = [&]() {
    static_for<ROUNDS>([&](auto rc) {
      cx<T> *const lrow = lds + (rc * RPR + rloc) * LROWX;
      cx<T> x[E];
      static_for<E>([&](auto q) { x[q] = lrow[lds_pad(tid + TP * q)]; });
      __syncthreads();  // the first pass scatters into the same rows
      fft_passes<T, 8, true>(x, lrow, twf, tid);  // natural order in LDS
    });
    __syncthreads();
  };
  transform_rows();
  // E in output layout: element (k, j), k = seg + SPI ic, rows j4 .. j4 + 3
  cx<T> ev[NOUT][4];
  static_for<NOUT>([&](auto ic) {
    const cx<T> *const d = lds + j4 * LROWX + lds_pad(seg + SPI * ic);
    static_for<4>([&](auto jc) { ev[ic][jc] = d[jc * LROWX]; });
  });
  __syncthreads();
  static_for<NIN>([&](auto ic) {
    cx<T> *const d = lds + (lrow0 + 2 * ic) * LROWX + lds_pad(me);
    d[0] = od[ic][0];
    d[1] = od[ic][1];
  });
  __syncthreads();
  transform_rows();

  // row i = j4 + jc, output k goes to out[base + t0 + i + k * out_stride]: 32 consecutive rows = 128-byte segments
  const size_t obase = base + (size_t)(t0 + j4);
  static_for<NOUT>([&](auto ic) {
    constexpr int i = ic;
    const int k = seg + SPI * i;
    const cx<T> *const d = lds + j4 * LROWX + lds_pad(k);
    const cx<T> w = mul_w16<T, i>(wseg);  // W_512^(seg + 32 i)
    cx<T> lo[4], hi[4];
    static_for<4>([&](auto jc) {
      const cx<T> tt = cmul(d[jc * LROWX], w);
      lo[jc] = (ev[i][jc] + tt) * scale;
      hi[jc] = (ev[i][jc] - tt) * scale;
    });
    const size_t go = obase + (size_t)k * (size_t)g.out_stride, gh = go + (size_t)H * (size_t)g.out_stride;
    st_stream(V4{lo[0].x, lo[1].x, lo[2].x, lo[3].x}, reinterpret_cast<V4 *>(out_re + go));
    st_stream(V4{lo[0].y, lo[1].y, lo[2].y, lo[3].y}, reinterpret_cast<V4 *>(out_im + go));
    st_stream(V4{hi[0].x, hi[1].x, hi[2].x, hi[3].x}, reinterpret_cast<V4 *>(out_re + gh));
    st_stream(V4{hi[0].y, hi[1].y, hi[2].y, hi[3].y}, reinterpret_cast<V4 *>(out_im + gh));
  });
}

// ---- general four-step path: N = N1 * N2 with 32 <= N1 <= N2 = the largest single-pass size ---
// Input index n = n1*N2 + n2, output index k = k1 + N1*k2; both factors run on the row kernels,
// so the data is transposed between them (Bailey's four-step):
//   1  [n1][n2] -> [n2][n1]                       (this kernel; window / zero padding of real frames here)
//   2  N1-point rows, in place                     (fft_stockham_kernel)
//   3  [n2][k1] -> [k1][n2], times W_N^{n2*k1}     (this kernel, TW)
//   4  N2-point rows, in place
//   5  [k1][k2] -> [k2][k1] = natural order        (this kernel; 1/N of the inverse, or AMP: the
//      amplitude / phase rows of spectrum())
// Five passes over HBM -- a completeness path for long one-shot transforms, not a bench configuration.
// One 256-thread workgroup moves one 32x32 tile of both planes through LDS, so the loads are
// unit-stride along the input rows and the stores along the output rows.
//   in: [batch][R][C] planar, element n = r*C + c; reads as zero for n >= used (real frames shorter
//   than N); in_im may be null (real input); win (N values) may be null.
template <typename T, bool TW, bool AMP>
__global__ void __launch_bounds__(256)
bigfft_transpose_kernel(const T *__restrict__ in_re, const T *__restrict__ in_im, const T *__restrict__ win,
                        const long long used, const long long in_stride,
                        const typename vec2<T>::type *__restrict__ twa, const typename vec2<T>::type *__restrict__ twb,
                        T *__restrict__ o1, T *__restrict__ o2, const int R, const int C, const T scale, const int bins,
                        const int nyq, const T s_edge, const T s_mid) {
  __shared__ T tre[32][33], tim[32][33];
  const int tiles_c = C / 32, tiles_r = R / 32;
  const long long blk = (long long)blockIdx.x;
  const long long b = blk / ((long long)tiles_r * tiles_c);
  const int t = (int)(blk % ((long long)tiles_r * tiles_c));
  const int tr = t / tiles_c, tc = t % tiles_c;
  const int tx = (int)threadIdx.x & 31, ty = (int)threadIdx.x >> 5;
  const T *const bre = in_re + (size_t)b * (size_t)in_stride;
  const T *const bim = in_im ? in_im + (size_t)b * (size_t)in_stride : nullptr;
  static_for<4>([&](auto ic) {
    const int r = tr * 32 + ty + 8 * ic, c = tc * 32 + tx;
    const long long n = (long long)r * C + c;
    const long long nc = n < used ? n : used - 1;  // unconditional clamped loads + select
    cx<T> v{bre[nc], bim ? bim[nc] : T(0)};
    if (win) v = v * win[n];
    if (n >= used) v = cx<T>{T(0), T(0)};
    if constexpr (TW) {
      const unsigned m = (unsigned)r * (unsigned)c;  // < N <= 2^28
      v = cmul(v, cmul(reinterpret_cast<const cx<T> *>(twa)[m >> 9], reinterpret_cast<const cx<T> *>(twb)[m & 511]));
    }
    tre[ty + 8 * ic][tx] = v.x;
    tim[ty + 8 * ic][tx] = v.y;
  });
  __syncthreads();
  static_for<4>([&](auto ic) {
    const int orow = tc * 32 + ty + 8 * ic, ocol = tr * 32 + tx;  // output matrix is [C][R]
    const cx<T> v{tre[tx][ty + 8 * ic], tim[tx][ty + 8 * ic]};
    const long long k = (long long)orow * R + ocol;
    if constexpr (AMP) {
      if (k < bins) {
        const size_t o = (size_t)b * (size_t)bins + (size_t)k;
        o1[o] = mag(v) * ((k == 0 || k == nyq) ? s_edge : s_mid);
        if (o2) o2[o] = T(atan2(v.y, v.x));
      }
    } else {
      const size_t o = (size_t)b * (size_t)R * (size_t)C + (size_t)k;
      o1[o] = v.x * scale;
      o2[o] = v.y * scale;
    }
  });
}

}  // namespace pdsp

// pdsp_fft2d_kernel.h -- the transform over the last two axes of [batch][H][W]: an LDS-resident image kernel and the
// column pass of the two-pass path.
//
// A 2-D transform of H x W points is the pass set of an H*W-point transform without the inter-pass twiddles and without
// the output transposition: W-point transforms along the rows, then H-point transforms down the columns.
//   X[k][l] = sum_h sum_w x[h][w] exp(-2 pi i (h k / H + w l / W))
// Images are contiguous planar complex: row stride W, image stride H*W, 16-byte aligned planes.  Both kernels run the
// forward transform; the callers swap planes for the inverse and pass the norm's scale, applied once in the last store.
//
// Alignment of the 4-wide accesses (V4 below): the boundary guarantees 16 bytes, and with W a multiple of 16 every
// access of a plane stays on a 16-byte boundary.  In f64 V4 is 32 bytes wide and nominally 32-byte aligned; only 16 is
// given.  That is enough: the compiler emits such an access as two global_load / global_store_dwordx4, which the
// hardware requires to be 4-byte aligned only, and nothing here derives an address from the nominal alignment (the f64
// instantiations of fft_staged_kernel and tile_pass_kernel make the same accesses).
#pragma once

#include "pdsp_fft_core.h"

namespace pdsp {

// ---- resident path: H*W <= 4096, one launch, one pass over HBM ------------------------------------------------------
// A 256-thread workgroup holds 4096 points -- IMGS = 4096 / (H*W) whole images, sixteen points per thread -- in the
// (4096 + 256)-element buffer of fft_stockham_kernel<12>: one pad element every 16 (lds_pad).  Its images are one
// contiguous 4096-point chunk per plane, so it moves them with coalesced 16-byte accesses on both sides, as
// fft_staged_kernel does with its rows.
//   load    point p of the chunk -> lds[lds_pad(p)] (natural layout: image, row h, column w).  A null imaginary plane is a
//           run-time (wave-uniform) select: no load, zeros.  Images past the batch (the last workgroup) are zeros: their
//           lanes load nothing and store nothing.
//   rows    the 4096 / W rows are padded LDS rows of LROW = W + W/16 elements (W is a multiple of 16).  W >= 64: W/16
//           threads per row, all rows at once, fft_passes.  W = 16, 32: one thread per row, fft_reg (W = 32: half the
//           threads).
//   columns H = 16, 32: one thread per column reads it out of the natural layout (lanes along w: conflict-free), runs
//           fft_reg and puts it back; the store reads 4 adjacent points.
//           H >= 64: the row pass leaves its result TRANSPOSED -- column c = image * W + w is the padded LDS row
//           lds + c * (H + H/16), again 4096 + 256 elements in all -- from its registers (one LDS trip, not two), H/16
//           threads per column run fft_passes on it, and the store gathers 4 adjacent columns per lane.
// The one-pad-per-16 layout is kept for both orientations.  The two transposing steps (the scatter into columns and the
// gather out of them) step by H + H/16 elements between lanes or between a lane's four points and take bank conflicts
// that the passes themselves do not; an odd column pitch would remove them but needs more than 4096 + 256 elements.
//   tww / twh = radix tables of the W- and H-point transforms (unused where fft_reg runs the axis).
// In place (re_out == re_in, im_out == im_in or im_in null): a workgroup loads all of its images before its first
// barrier and stores only into them.
template <typename T, int LH, int LW>
__global__ void __launch_bounds__(256)
fft2d_resident_kernel(const T *re_in, const T *im_in, T *re_out, T *im_out,
                      const typename vec2<T>::type *__restrict__ tww, const typename vec2<T>::type *__restrict__ twh,
                      const T scale, const long long batch) {
  constexpr int H = 1 << LH, W = 1 << LW, HW = H * W, CHUNK = 4096, WG = 256;
  static_assert(LH >= 4 && LW >= 4 && LH + LW <= 12, "16 <= H, W and H*W <= 4096");
  using TW = FftTraits<LW>;
  using TH = FftTraits<LH>;
  constexpr bool ROW_REG = LW <= 5, COL_REG = LH <= 5;
  constexpr int ROWS = CHUNK / W, NCOLS = CHUNK / H;  // rows and columns of the workgroup's images
  constexpr int LCOL = H + H / 16;                     // pitch of the transposed layout
  typedef T V4 __attribute__((ext_vector_type(4)));
  __shared__ cx<T> lds[CHUNK + CHUNK / 16];

  const int t = (int)threadIdx.x;
  const size_t base = (size_t)blockIdx.x * CHUNK;
  const size_t limit = (size_t)batch * HW;  // points per plane: a multiple of 4, and a group of 4 lies in one image
  const bool has_im = im_in != nullptr;

  static_for<CHUNK / 4 / WG>([&](auto ic) {
    const int p = 4 * (t + WG * ic);
    const size_t g = base + (size_t)p;
    V4 r = V4{T(0), T(0), T(0), T(0)}, m = V4{T(0), T(0), T(0), T(0)};
    if (g < limit) {
      r = ld_stream(reinterpret_cast<const V4 *>(re_in + g));
      if (has_im) m = ld_stream(reinterpret_cast<const V4 *>(im_in + g));
    }
    cx<T> *const d = lds + lds_pad(p);  // 4 points never straddle a 16-block
    d[0] = cx<T>{r.x, m.x};
    d[1] = cx<T>{r.y, m.y};
    d[2] = cx<T>{r.z, m.z};
    d[3] = cx<T>{r.w, m.w};
  });
  // the tables behind the image loads (load_order_fence's header)
  RegTwiddles<T, ROW_REG ? 6 : LW> twfw;
  RegTwiddles<T, COL_REG ? 6 : LH> twfh;
  if constexpr (!ROW_REG) twfw.load(reinterpret_cast<const cx<T> *>(tww), t % TW::TP);
  // (beside a 32-point register row the column bases would cost f32 128 x 32 its fourth workgroup per CU: 134 VGPRs;
  // there they are fetched after the rows)
  constexpr bool TWH_EARLY = !COL_REG && LW != 5;
  if constexpr (TWH_EARLY) twfh.load(reinterpret_cast<const cx<T> *>(twh), t % TH::TP);
  __syncthreads();

  // ---- W-point transforms along the rows; result natural (COL_REG) or transposed
  if constexpr (ROW_REG) {
    const bool holds_row = t < ROWS;  // whole waves: W = 32 leaves waves 2 and 3 idle
    const int img = t / H, h = t % H;
    cx<T> a[W];
    if (holds_row) {
      static_for<W>([&](auto q) { a[q] = lds[lds_pad(t * W + q)]; });
      fft_reg<T, W>(a);  // X[l] in slot bitrev(l)
    }
    __syncthreads();  // the transposed layout overwrites other threads' rows
    if (holds_row) {
      static_for<W>([&](auto l) {
        if constexpr (COL_REG) lds[lds_pad(t * W + l)] = a[bitrev(l, LW)];
        else lds[(img * W + l) * LCOL + lds_pad(h)] = a[bitrev(l, LW)];
      });
    }
  } else {
    constexpr int TP = TW::TP;
    const int tid = t % TP, r = t / TP;  // 256 / TP == ROWS: every row at once
    cx<T> *const lrow = lds + r * TW::LROW;
    cx<T> x[TW::E];
    fft_pass_readback<T, LW, 4>(x, lrow, tid);
    __syncthreads();  // the first pass scatters into the same rows
    fft_passes<T, LW, COL_REG>(x, lrow, twfw, tid);
    if constexpr (!COL_REG) {
      __syncthreads();  // every thread holds X[tid + TP q] of its row: the buffer now takes the columns
      const int img = r / H, h = r % H;
      static_for<TW::E>([&](auto q) { lds[(img * W + tid + TP * q) * LCOL + lds_pad(h)] = x[q]; });
    }
  }
  __syncthreads();

  // ---- H-point transforms down the columns
  if constexpr (COL_REG) {
    if (t < NCOLS) {
      const int img = t / W, w = t % W;
      cx<T> *const col = lds + cpad(img * HW) + lds_pad(w);  // pad(img HW + h W + w) = cpad(img HW) + cpad(h W) + pad(w)
      cx<T> a[H];
      static_for<H>([&](auto hc) { a[hc] = col[cpad(hc * W)]; });
      fft_reg<T, H>(a);
      static_for<H>([&](auto k) { col[cpad(k * W)] = a[bitrev(k, LH)]; });  // the thread's own column
    }
  } else {
    constexpr int TP = TH::TP;
    const int tid = t % TP, c = t / TP;  // 256 / TP == NCOLS
    cx<T> *const lcol = lds + c * LCOL;
    cx<T> x[TH::E];
    if constexpr (!TWH_EARLY) twfh.load(reinterpret_cast<const cx<T> *>(twh), tid);
    fft_pass_readback<T, LH, 4>(x, lcol, tid);
    __syncthreads();
    fft_passes<T, LH, true>(x, lcol, twfh, tid);  // natural order along the column
  }
  __syncthreads();

  static_for<CHUNK / 4 / WG>([&](auto ic) {
    const int p = 4 * (t + WG * ic);
    const size_t g = base + (size_t)p;
    if (g < limit) {
      cx<T> v[4];
      if constexpr (COL_REG) {
        const cx<T> *const d = lds + lds_pad(p);
        static_for<4>([&](auto j) { v[j] = d[j] * scale; });
      } else {
        const int img = p / HW, k = (p / W) % H, w = p % W;
        const cx<T> *const d = lds + (img * W + w) * LCOL + lds_pad(k);
        static_for<4>([&](auto j) { v[j] = d[j * LCOL] * scale; });
      }
      st_stream(V4{v[0].x, v[1].x, v[2].x, v[3].x}, reinterpret_cast<V4 *>(re_out + g));
      st_stream(V4{v[0].y, v[1].y, v[2].y, v[3].y}, reinterpret_cast<V4 *>(im_out + g));
    }
  });
}

// ---- two-pass path: the column pass, in place on the output planes ---------------------------------------------------
// The rows have been transformed by the row kernels (run_complex on batch * H rows of W points).  Both kernels below
// read ALL of a workgroup's columns before they store any of them, and the workgroups' column sets are disjoint: that is
// why the pass is safe in place.

// H = 64 ... 512: a 256-thread workgroup owns TILE adjacent columns of one image -- tile_pass_kernel's COLS geometry
// with the twiddle products, the block / permutation options and the transposed store taken out.  Element (p, j), p < H,
// j < TILE, is plane[b H W + p W + t0 + j]; it moves between HBM and LDS in row segments of TILE elements (16-byte
// accesses, 256 / (TILE / 4) segments per access of the workgroup), column j is LDS row j at a pitch of LROWX elements
// (tile_pass_kernel's header: four rows of LROW would land on the same banks), and the H-point transforms run on those
// rows, 256 / (H / 16) at a time.
//   tw = radix table of the H-point transform; tiles = W / TILE.
template <typename T, int LH, int TILE>
__global__ void __launch_bounds__(256)
fft2d_cols_tile_kernel(T *re, T *im, const typename vec2<T>::type *__restrict__ tw, const int w, const int tiles,
                       const T scale, const long long batch) {
  using TR = FftTraits<LH>;
  constexpr int L = TR::N, E = TR::E, TP = TR::TP, RPR = 256 / TP, ROUNDS = TILE / RPR;
  static_assert(LH >= 6 && LH <= 9 && TILE % RPR == 0 && TILE % 4 == 0 && ROUNDS >= 1, "tile of whole rounds");
  constexpr int LROWX = TR::LROW + ((2 - TR::LROW % 8) + 8) % 8;
  constexpr int TS = TILE / 4, SPI = 256 / TS;  // threads per tile segment, segments per access of the workgroup
  static_assert(L % SPI == 0, "whole accesses");
  typedef T V4 __attribute__((ext_vector_type(4)));
  __shared__ cx<T> lds[TILE * LROWX];

  const int t = (int)threadIdx.x;
  const long long b = (long long)blockIdx.x / tiles;
  const int t0 = (int)((long long)blockIdx.x % tiles) * TILE;
  if (b >= batch) return;
  const int seg = t / TS, j4 = (t % TS) * 4;
  const size_t base = (size_t)b * (size_t)L * (size_t)w + (size_t)(t0 + j4);

  static_for<L / SPI>([&](auto ic) {
    const int p = seg + SPI * ic;
    const size_t gi = base + (size_t)p * (size_t)w;
    const V4 r = ld_stream(reinterpret_cast<const V4 *>(re + gi));
    const V4 m = ld_stream(reinterpret_cast<const V4 *>(im + gi));
    cx<T> *const d = lds + j4 * LROWX + lds_pad(p);
    d[0 * LROWX] = cx<T>{r.x, m.x};
    d[1 * LROWX] = cx<T>{r.y, m.y};
    d[2 * LROWX] = cx<T>{r.z, m.z};
    d[3 * LROWX] = cx<T>{r.w, m.w};
  });
  const int tid = t % TP, rloc = t / TP;
  RegTwiddles<T, LH> twf;
  twf.load(reinterpret_cast<const cx<T> *>(tw), tid);
  __syncthreads();  // the whole tile is in LDS: nothing of it is read from HBM after this point

  static_for<ROUNDS>([&](auto rc) {
    cx<T> *const lrow = lds + (rc * RPR + rloc) * LROWX;
    cx<T> x[E];
    fft_pass_readback<T, LH, 4>(x, lrow, tid);
    __syncthreads();  // the first pass scatters into the same rows
    fft_passes<T, LH, true>(x, lrow, twf, tid);  // natural order in LDS
  });
  __syncthreads();

  static_for<L / SPI>([&](auto ic) {
    const int p = seg + SPI * ic;
    const cx<T> *const d = lds + j4 * LROWX + lds_pad(p);
    const cx<T> v0 = d[0 * LROWX] * scale, v1 = d[1 * LROWX] * scale, v2 = d[2 * LROWX] * scale, v3 = d[3 * LROWX] * scale;
    const size_t go = base + (size_t)p * (size_t)w;
    st_stream(V4{v0.x, v1.x, v2.x, v3.x}, reinterpret_cast<V4 *>(re + go));
    st_stream(V4{v0.y, v1.y, v2.y, v3.y}, reinterpret_cast<V4 *>(im + go));
  });
}

// H = 16, 32: one thread per column with fft_reg, as fourstep_cols_kernel does for its short factor.  A workgroup owns
// 256 adjacent columns of one image (the two-pass path has W >= 256 at these heights); loads and stores are unit-stride
// across the lanes.  A thread holds its whole column before it stores.
template <typename T, int LH>
__global__ void __launch_bounds__(256)
fft2d_cols_reg_kernel(T *re, T *im, const int w, const T scale, const long long batch) {
  constexpr int H = 1 << LH;
  static_assert(LH == 4 || LH == 5, "H = 16, 32");
  const int cblocks = w / 256;
  const long long b = (long long)blockIdx.x / cblocks;
  const int col = (int)((long long)blockIdx.x % cblocks) * 256 + (int)threadIdx.x;
  if (b >= batch) return;
  const size_t base = (size_t)b * (size_t)H * (size_t)w + (size_t)col;
  cx<T> a[H];
  static_for<H>([&](auto q) {
    const size_t i = base + (size_t)q * (size_t)w;
    a[q] = cx<T>{ld_stream(re + i), ld_stream(im + i)};
  });
  fft_reg<T, H>(a);
  static_for<H>([&](auto k) {
    const cx<T> v = a[bitrev(k, LH)] * scale;
    const size_t i = base + (size_t)k * (size_t)w;
    st_stream(v.x, re + i);
    st_stream(v.y, im + i);
  });
}

}  // namespace pdsp

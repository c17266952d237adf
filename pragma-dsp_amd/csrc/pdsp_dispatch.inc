// pdsp_dispatch.inc -- kernel dispatch by size and call shape (templates on the scalar type T), included by the
// kernel translation units (pdsp_kernels_*.hip), which instantiate it explicitly; see pdsp_internal.h.
#include <climits>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "pdsp_internal.h"
#include "pdsp_fft_kernel.h"

namespace pdsp_host {

// Are all the pointers multiples of `bytes` (a power of two)?  Null pointers are.
template <class... P>
bool aligned(size_t bytes, const P *...p) {
  return (((uintptr_t)p | ...) & (bytes - 1)) == 0;
}

// A window that is one of the plan's own tables (pdsp_plan_window_f32) is known by kind (-1: the caller's table;
// PDSP_WIN_RECT is all ones).  The kinds that are cosine sums w = k0 + k1 cos(f n) + k2 cos^2(f n) have a term
// count (2 / 3; 0: none) and coefficients, for the kernels that evaluate them in registers.
template <typename T>
int window_kind(const Tables<T> &t, const T *window) {
  int kind = -1;
  for (int k = 0; k < 4; ++k)
    if (window && window == t.win[k]) kind = k;
  return kind;
}
struct CosineSum {
  int terms = 0;
  float k0 = 0.f, k1 = 0.f, k2 = 0.f;
};
inline CosineSum cosine_sum(int kind) {
  if (kind == PDSP_WIN_HANN) return {2, 0.5f, -0.5f, 0.f};
  if (kind == PDSP_WIN_HAMMING) return {2, 0.54f, -0.46f, 0.f};
  if (kind == PDSP_WIN_BLACKMAN) return {3, 0.42f - 0.08f, -0.5f, 2 * 0.08f};
  return {};
}

// t.twa / t.twb as the kernels take them: W_N^m = a[m >> 9] * b[m & 511]
template <typename T>
struct TwAB {
  const pdsp::cx<T> *a, *b;
};
template <typename T>
TwAB<T> twab(const Tables<T> &t) {
  return {reinterpret_cast<const pdsp::cx<T> *>(t.twa), reinterpret_cast<const pdsp::cx<T> *>(t.twb)};
}

// Peaks-only output: the amplitude / phase rows the peak kernels read but the caller did not ask for live in
// scratch, `rows` values each.  peak_rows_extra: the values that takes; place_peak_rows points amp / ph at them.
inline size_t peak_rows_extra(const void *peaks, const void *amp, const void *ph, size_t rows) {
  return (peaks && !amp ? rows : 0) + (peaks && !ph ? rows : 0);
}
template <typename T>
void place_peak_rows(const void *peaks, T *&amp, T *&ph, T *at, size_t rows) {
  if (peaks && !amp) amp = at, at += rows;
  if (peaks && !ph) ph = at;
}

// Do any of the output planes share bytes with any of the input planes?  Byte ranges, not pointer equality: an
// output that starts one row into the input buffer overlaps it too.  The multi-pass paths use the output planes as
// their first scratch pair only when this is false.
template <typename T>
bool planes_overlap(const T *re_in, const T *im_in, const T *re_out, const T *im_out, size_t plane_bytes) {
  auto hit = [&](const T *a, const T *b) { return host_ranges_overlap(a, plane_bytes, b, plane_bytes); };
  return hit(re_in, re_out) || hit(re_in, im_out) || hit(im_in, re_out) || hit(im_in, im_out);
}

// ---- the decision ------------------------------------------------------------------------------------------------
// What one pdsp_fft_* / pdsp_spectrum_* call runs.  pick_transform and pick_spectrum choose it from the plan's tables,
// the call's shape and pointers, and the development switches; they make no HIP call and change nothing, and they are
// the only place in this file that reads a switch or asks whether a table exists.  run_complex and spectrum_impl are
// argument checks -> pick -> a switch on the path; pdsp_dev_transform_path_* / pdsp_dev_spectrum_path_* run the same
// checks and the same pick and copy the struct out (include/pdsp_hip_dev.h documents the fields in this order).
enum Path {
  kNothing = 0,  // an empty batch
  // transforms; 2 ... 5 also name the rows kernel of a row pass (Pick::rows, Pick::n1_rows)
  kTinyStaged = 1, kStaged, kStockham, kSplit2, kSplit4, kRealPacked, kPaired, kTilePasses, kFourstepFused, kFourstepGeneral,
  // spectra (the two four-step forms are shared)
  kSpecMemset, kSpecTiles, kSpecStaged, kSpecDif16k, kSpecPacked, kSpecTiny, kSpecSmall
};
enum Tile { kTilePlain = 1, kTileCols512, kTileRows512 };            // the kernel of one tile pass
enum Head { kHeadChain = 0, kHeadSplit4, kHeadPaired };             // kSpecTiles: what runs the N/2-point transform
enum Peaks { kPeakWave = 1, kPeakFind = 2, kPeakFromRows = 4 };     // the peak kernels behind the stored rows (bits)
struct Pick {
  int path = kNothing;
  int rows = 0;        // single-pass paths: == path; four-step forms: the kernel of the N2-point rows
  int n1_rows = 0;     // general four-step: the kernel of the N1-point rows ...
  int n1_square = 0;   // ... 1: N1 == N2, on the N2-point tables; 0: on the tables of their own (Tables::tw1)
  int np = 0;          // tile passes (kTilePasses, kSpecTiles with kHeadChain): how many, and each one's kernel
  int tile[3] = {0, 0, 0};
  int tile_major = 0;  // three passes: the planes between the first two tile-major (TileGeom::perm_*), not natural
  int pairs = 0;       // scratch plane pairs drawn
  int out_first = 0;   // the output planes serve as the first intermediate pair
  int fast = 0;        // kSpecStaged / kSpecDif16k / kSpecPacked: whole pair-aligned one-sided frames, no phase rows
  int wmode = 0;       // the same paths: 0 rect, 1 window table, 2 / 3 fused two- / three-term cosine sum
  int first = 0;       // kSpecTiles: the first pass's loader, 3 rect, 4 window table, 5 / 6 fused cosine sum
  int fused_peaks = 0; // kSpecDif16k / kSpecPacked: the peak records come from the spectrum kernel itself
  int peaks = 0;       // the tail
  int head = kHeadChain;
};
static_assert(sizeof(Pick) == PDSP_DEV_PATH_INFO * sizeof(int), "pdsp_hip_dev.h documents Pick field by field");

// Rows of planar complex points: N = 16384 (f32) goes to fft_split4_kernel when the input planes allow 16-byte
// loads, N = 8192 to fft_split2_kernel, everything else to the single-pass kernel of its size.
// N = 8192: measured on one box, f64 C2C 4.35 -> 5.80 TB/s, f64 real-in 4.0 -> 5.6, f32 real-in 5.4 -> 5.7,
// f32 C2C a wash (stays on the single-pass kernel)
// (f64 real rows run on fft_real_kernel; their LoadReal form of this kernel spilled 37 registers and is not built)
template <typename T>
int pick_rows(const Tables<T> &t, int log2n, bool has_im, bool aligned16) {
  constexpr bool f32 = sizeof(T) == 4;
  if (f32 && log2n == 14 && g_split16k && aligned16 && t.tws4 && t.tw12) return kSplit4;
  if ((f32 || has_im) && log2n == 13 && (!f32 || !has_im || g_split8k_f32) && g_split16k && aligned16 && t.tws2 && t.tw12)
    return kSplit2;
  return kStockham;
}

// The row passes of the general four-step path (bigfft_rows); its scratch planes are aligned.
template <typename T>
void pick_general(const Tables<T> &t, Pick &p) {
  p.n1_square = t.log2n1 == t.log2n2;
  if (p.n1_square) p.n1_rows = pick_rows<T>(t, t.log2n1, true, true);
  // short rows: the staged kernel's coalesced I/O
  else p.n1_rows = (t.log2n1 <= (sizeof(T) == 4 ? 8 : 7) && g_staged_small) ? kStaged : kStockham;
  p.rows = pick_rows<T>(t, t.log2n2, true, true);
}

// The kernel of each of np tile passes over the factors 2^l[i] (tilepass_chain); `first` = the first pass's loader.
// A 512-point factor runs on 32-wide tiles where its kernels' table exists (f32): tile_cols512_kernel as a column pass
// (128-byte strided segments; complex or plain real rows only), tile_rows512_kernel as the last pass (128-byte output
// segments), instead of tile_pass_kernel's 16-wide ones.  Three passes keep the planes between the first two
// tile-major, so that the second pass reads its [B][TILE] tiles as contiguous chunks.  pdsp_set_twopass bit 1 keeps
// the plain tiles and the natural order (A/B tests).
template <typename T>
void pick_tiles(const Tables<T> &t, int np, const int *l, int first, Pick &p) {
  const bool wide = sizeof(T) == 4 && t.tw8 && !(g_twopass & 2);
  int lsum = 0;
  for (int i = 0; i < np; ++i) lsum += l[i];
  p.np = np;
  for (int i = 0, before = 0; i < np; before += l[i++]) {
    const bool last = i == np - 1;
    // 16-wide tiles of this pass: across the columns behind the factor, or for the last pass the rows in front
    const long long tiles = (1LL << (last ? before : lsum - before - l[i])) / tile_width(l[i]);
    const bool wide_here = wide && l[i] == 9 && tiles % 2 == 0 && (i > 0 || first <= 1);
    p.tile[i] = !wide_here ? kTilePlain : (last ? kTileRows512 : kTileCols512);
  }
  p.tile_major = np == 3 && !(g_twopass & 2);
}

template <typename T>
Pick pick_transform(const pdsp_plan *plan, long long batch, const T *re_in, const T *im_in, const T *re_out,
                    const T *im_out, bool by_size = false) {
  const Tables<T> &t = tables<T>(plan);
  const int L = plan->log2n;
  Pick p;
  auto aliased = [&] {
    return planes_overlap(re_in, im_in, re_out, im_out, (size_t)batch * (size_t)plan->n * sizeof(T));
  };
  // f64 Radix2Fft.forward rows (real input; f64 is the drop-in's default arithmetic) of N = 8192 and 16384: one
  // N/2-point packed-real transform per row and the split to X[k], X[k + N/2] (fft_real_kernel) -- half the
  // butterflies of the complex kernel on (x, 0), the same store streams, and N = 16384 stays in one pass.  These are
  // the sizes where the complex f64 kernel is short of registers (N = 8192: fft_split2_kernel's LoadReal form
  // spilled) or does not exist (N = 16384: four-step): tools/ab_real_packed.py --f64 on two boxes, N = 8192
  // 4.93 -> 6.57 and 3.97 -> 5.69 TB/s, N = 16384 1.60 -> 5.18 and 1.57 -> 5.07; one frame through the host drop-in
  // (tools/ab_single_frame_latency.py) 39.7 -> 36.2 us at 8192, but 47.3 -> 50.1 us at 16384 (one 512-thread
  // workgroup is a longer critical path than three short launches), hence the batch threshold there.  Below 8192
  // the same kernel measured +1 ... +9 % on one box and -9 ... +2 % on another (and 3-7 % slower for one frame): not
  // robust, not dispatched, not built.  In f32 it measured 0.98 ... 1.01 of the complex kernels: not built either.
  // Rows aligned to a sample pair.
  // by_size: the host forms (transform_host), which promise that a row's bits depend neither on the rows that travel
  // with it nor on how the call is cut into chunks -- there N = 16384 runs this kernel at every row count (DESIGN.md
  // 4.1d has the times); the batch threshold is the device forms' alone.
  if (sizeof(T) == 8 && !im_in && g_real_packed && (L == 13 || (L == 14 && (by_size || batch >= 8))) && t.tw_half && t.twr &&
      aligned(2 * sizeof(T), re_in)) {
    p.path = kRealPacked;
    return p;
  }
  if (sizeof(T) == 4 && (t.tp_np || L == 15 || L == 16) && aligned(16, re_in, im_in, re_out, im_out)) {
    // N = 2^15 / 2^16 out of place: ONE pass over HBM by 2 / 4 sibling workgroups per transform that share their
    // XCD's L2 (fft_paired_kernel).  In place the siblings would overwrite each other's input: tile passes then.
    // pdsp_set_twopass: any value but 1 keeps the tile passes (5: their current form) -- A/B tests.
    if ((L == 15 || L == 16) && g_twopass == 1 && t.tw12 && t.tws4 && t.twa && t.twb && !aliased()) {
      p.path = kPaired;
      return p;
    }
    // tile passes with balanced factors (two for 2^15..2^18, three for 2^19..2^27) where the tables exist and
    // every plane is 16-byte aligned; pdsp_set_twopass(0) keeps round 1's four-step forms (A/B tests).
    // Two passes: one scratch pair.  Three passes: the output planes double as the first scratch pair
    // unless they share bytes with the input (equal pointers or a partial overlap).
    if (t.tp_np && (g_twopass & 1)) {
      p.path = kTilePasses;
      pick_tiles<T>(t, t.tp_np, t.tp_l, im_in ? 0 : 1, p);
      p.out_first = t.tp_np == 3 && !aliased();
      p.pairs = t.tp_np == 3 && !p.out_first ? 2 : 1;
      return p;
    }
  }
  if (t.log2n1 > pdsp::kMaxLog2N1) {  // general four-step: the output planes double as the first scratch pair
    p.path = kFourstepGeneral;
    pick_general<T>(t, p);
    p.out_first = !aliased();
    p.pairs = p.out_first ? 1 : 2;
    return p;
  }
  if (t.log2n1 > 0) {  // beyond the single-pass limit: four-step through stream-ordered scratch planes
    p.path = kFourstepFused;
    p.rows = pick_rows<T>(t, t.log2n2, true, true);  // scratch planes are aligned
    p.pairs = 1;
    return p;
  }
  const bool planes16 = aligned(4 * sizeof(T), re_in, im_in, re_out, im_out);
  if (L >= 1 && L <= 4 && g_staged_small && planes16) {  // 2 <= N <= 16: one thread per row
    p.path = kTinyStaged;
    return p;
  }
  // small N: coalesced 16-byte I/O staged through LDS (fft_staged_kernel)
  // (f64 at N = 256: 69.6 KB of LDS per workgroup, the direct kernel measures 12 % faster)
  if (L >= 5 && L <= (sizeof(T) == 4 ? 8 : 7) && g_staged_small && planes16) {
    p.path = kStaged;
    return p;
  }
  p.path = p.rows = pick_rows<T>(t, L, im_in != nullptr, aligned(16, re_in, im_in));
  return p;
}

// The peak kernels behind stored amplitude rows of `bins` values: an index array (idx) and / or records (recs).
inline int pick_peaks(int bins, bool idx, bool recs) {
  if (bins <= 2048) return idx || recs ? kPeakWave : 0;  // one wave per row
  return (idx ? kPeakFind : 0) | (recs ? kPeakFromRows : 0);
}

// The arguments are spectrum_impl's after its checks; frame_len > 0 or the path is kSpecMemset.
template <typename T>
Pick pick_spectrum(const pdsp_plan *plan, const T *frames, long long frame_len, long long frame_stride, const T *window,
                   int sides, const T *amp_out, const T *phase_out, const int32_t *peak_idx_out,
                   const pdsp_peak32 *peaks_out) {
  constexpr bool f32 = sizeof(T) == 4;
  const Tables<T> &t = tables<T>(plan);
  const long long n = plan->n;
  const int L = plan->log2n;
  const int bins = (int)(sides == PDSP_SIDES_ONE ? n / 2 + 1 : n);
  const long long used = frame_len < n ? frame_len : n;
  const int kind = f32 ? window_kind(t, window) : -1;  // (f64 reads every window as a table)
  Pick p;
  if (used == 0) {  // an empty frame is all zeros: amplitude 0, atan2(0, 0) = 0, peak 0
    p.path = kSpecMemset;
    return p;
  }
  // N beyond the single-pass limit, whole 16-byte aligned frames: the packed-real form on tile passes.
  // z[m] = (x*w)[2m] + i (x*w)[2m+1] is read straight from the frame (and the window table) by the first
  // pass; two (N <= 2^18) or three passes of the N/2-point transform; split_amp_rows_kernel undoes the packing on
  // the way to the amplitude (+ phase) rows.  HBM bytes per sample: 4+4, 4+4 (, 4+4), 4+2 = 22 (30) where the
  // four-step forms on (x*w, 0) move 38 (70).  The four-step forms stay for partial / unaligned frames and f64.
  if (f32 && t.log2n1 > 0 && t.hp_np && (g_twopass & 1) && used == n && (frame_stride & 3) == 0 &&
      aligned(16, frames, window)) {
    p.path = kSpecTiles;
    p.pairs = 2;
    // a window that is one of the plan's own tables (pdsp_plan_window_f32) is known by kind: the cosine sum is
    // then evaluated in the first pass instead of being read back (4 more bytes per sample).
    p.first = window && kind != PDSP_WIN_RECT ? 4 : 3;  // createWindow("rect") is all ones
    if (const int terms = cosine_sum(kind).terms; terms && t.hp_win && g_fused_window) p.first = terms == 2 ? 5 : 6;
    // N = 32768: the 16384-point transform is one pass of fft_split4_kernel (14 bytes per sample in all).
    // N = 65536: the 32768-point transform in ONE pass by two sibling workgroups per frame that share an XCD's
    // L2 (fft_paired_kernel, packed loader): 14 bytes per sample in all, where the two tile passes move 22
    if (L == 15 && t.tws4 && t.tw12 && g_split16k) p.head = kHeadSplit4;
    else if (L == 16 && g_twopass == 1 && t.tws4 && t.tw12) p.head = kHeadPaired;
    else pick_tiles<T>(t, t.hp_np, t.hp_l, p.first, p);
    p.peaks = pick_peaks(bins, peak_idx_out, peaks_out);
    return p;
  }
  // N beyond the single-pass limit: four-step on (x*w, 0), amplitude rows in the last pass.  (Not where the packed-real
  // tables exist: f64 frames of N = 16384 are ONE 8192-point packed transform -- spectrum_packed_kernel<double, 13> --
  // although the complex f64 transform of that size is a four-step one.  Round 2 sent them through the four-step
  // path by this test's order.)
  if (t.log2n1 > 0 && !t.tw_half) {
    if (t.log2n1 > pdsp::kMaxLog2N1) {  // general path: two scratch pairs
      p.path = kFourstepGeneral, p.pairs = 2;
      pick_general<T>(t, p);
    } else {
      p.path = kFourstepFused, p.pairs = 1;
      p.rows = pick_rows<T>(t, t.log2n2, true, true);
    }
    p.peaks = pick_peaks(bins, peak_idx_out, peaks_out);
    return p;
  }
  if (t.tw_half) {
    // packed-real path (N >= 64): N/2-point complex transform + Hermitian split (+ findPeak) fused with the store.
    // fast variant: whole pair-aligned frames (and window), one-sided, no phase rows (config 4's shape); the
    // general variant takes any frame length, stride and alignment of frames and window
    p.fast = aligned(2 * sizeof(T), frames, window) && (frame_stride & 1) == 0 && used == n &&
             sides == PDSP_SIDES_ONE && phase_out == nullptr;  // aligned to one (re, im) pair
    p.wmode = window ? 1 : 0;
    // 64 <= N <= 512, amplitude only: contiguous frames staged in / amplitude rows staged out through LDS
    // (f32 only: in f64 the two LDS regions take 102 KB, one workgroup per CU, and measure slower than the direct kernel)
    if (f32 && p.fast && !peaks_out && !peak_idx_out && L >= 6 && L <= 9 && g_staged_small && frame_stride == n &&
        aligned(4 * sizeof(T), frames, window)) {
      p.path = kSpecStaged;
      return p;
    }
    if (f32) {
      // A window that is one of the PLAN'S OWN tables (pdsp_plan_window_f32) is known by kind: the kernels
      // that can (whole f32 frames, N = 1024 ... 16384) then evaluate the cosine sum in registers.
      if (kind == PDSP_WIN_RECT) p.wmode = 0;  // createWindow("rect") is all ones
      if (const int terms = cosine_sum(kind).terms; terms && t.wf_base && g_fused_window && p.fast) p.wmode = terms;
      p.fused_peaks = peaks_out != nullptr;  // (f64 has no fused peaks, and no entry point that asks for records)
    }
    p.peaks = pick_peaks(bins, peak_idx_out, false);
    // N = 16384: two 4096-point sub-transforms per 256-thread workgroup (3 frames per CU instead of 2),
    // decimation in frequency on top (spectrum_dif16k_kernel).  A window that is one of the PLAN'S OWN
    // tables (pdsp_plan_window_f32) is known by kind, and createWindow is fused into the kernel: the
    // reference's windows are cosine sums (fourier.ts:14-52), evaluated in registers instead of being
    // read back, 64 KB per frame, from L2.  Any other window pointer is read as a table.
    if (f32 && p.fast && L == 14 && g_split16k && t.wf_base) {
      p.path = kSpecDif16k;
      return p;
    }
    // fused cosine-sum windows (wmode 2 / 3) on spectrum_packed_kernel: whole f32 frames of N = 1024 ... 8192 (the
    // sizes whose plans carry the angle-addition tables); everything else reads the window as a table
    p.path = kSpecPacked;
    if (p.wmode >= 2 && !(L >= 10 && L <= 13)) p.wmode = 1;
    return p;
  }
  // complex kernel on (x, 0) for N < 64 (the sizes without packed-real tables); peaks come from the stored rows.
  // 2 <= N <= 32, whole contiguous frames, amplitude only: one thread per frame, chunk staged through LDS
  if (L >= 1 && L <= 5 && g_staged_small && used == n && frame_stride == n && amp_out && !phase_out && !peaks_out &&
      aligned(4 * sizeof(T), frames)) {
    p.path = kSpecTiny;
    p.peaks = pick_peaks(bins, peak_idx_out, false);
    return p;
  }
  p.path = kSpecSmall;
  p.peaks = pick_peaks(bins, peak_idx_out, peaks_out);
  return p;
}

template <typename T, int LOG2N, class LD, class ST>
hipError_t launch_one(const LD &ld, const ST &st, const typename pdsp::vec2<T>::type *tw, long long batch,
                      hipStream_t s) {
  if constexpr (LOG2N > max_log2n<T>()) {
    return hipErrorInvalidValue;  // would not fit LDS; never instantiated
  } else {
    using TR = pdsp::FftTraits<LOG2N>;
    const long long blocks = (batch + TR::ROWS - 1) / TR::ROWS;
    hipLaunchKernelGGL((pdsp::fft_stockham_kernel<T, LOG2N, LD, ST>), dim3((unsigned)blocks), dim3(TR::WG), 0, s, ld,
                       st, tw, batch);
    return hipGetLastError();
  }
}

template <typename T, class LD, class ST>
hipError_t launch_fft(int log2n, const LD &ld, const ST &st, const typename pdsp::vec2<T>::type *tw, long long batch,
                      hipStream_t s) {
  return with_int<0, 14>(log2n, hipErrorInvalidValue, [&](auto L) { return launch_one<T, L>(ld, st, tw, batch, s); });
}

// The same for N <= 32 only (spectrum() of frames below the packed-real path's sizes: LoadFrameWindowed /
// StoreAmplitude are not instantiated for the sizes that never take them).
template <typename T, class LD, class ST>
hipError_t launch_fft_small(int log2n, const LD &ld, const ST &st, const typename pdsp::vec2<T>::type *tw, long long batch,
                            hipStream_t s) {
  return with_int<0, 5>(log2n, hipErrorInvalidValue, [&](auto L) { return launch_one<T, L>(ld, st, tw, batch, s); });
}

// Rows of planar complex points on the kernel pick_rows chose (kSplit4 / kSplit2 / kStockham).
template <typename T, class LD, class ST>
hipError_t launch_rows(int kernel, const Tables<T> &t, int log2n, const LD &ld, const ST &st, long long batch,
                       hipStream_t s) {
  if constexpr (sizeof(T) == 4) {
    if (kernel == kSplit4) {
      hipLaunchKernelGGL((pdsp::fft_split4_kernel<T, 12, LD, ST>), dim3((unsigned)batch), dim3(256), 0, s, ld, st,
                         t.tw12, t.tws4, batch);
      return hipGetLastError();
    }
  }
  if constexpr (!(sizeof(T) == 8 && !LD::kHasIm)) {  // (the f64 LoadReal form is not built: pick_rows)
    if (kernel == kSplit2) {
      hipLaunchKernelGGL((pdsp::fft_split2_kernel<T, LD, ST>), dim3((unsigned)batch), dim3(256), 0, s, ld, st, t.tw12,
                         t.tws2, batch);
      return hipGetLastError();
    }
  }
  return launch_fft<T>(log2n, ld, st, t.tw, batch, s);
}


template <typename T, int LOG2M>
hipError_t launch_packed_one(bool fast, const T *frames, const T *win, int wmode, pdsp::WinFused wf, long long frame_len,
                             long long stride, const typename pdsp::vec2<T>::type *tw,
                             const typename pdsp::vec2<T>::type *twr, T *amp, T *ph, int two_sided, T s_edge, T s_mid,
                             pdsp::PeakRec *peaks, T freq_scale, long long batch, hipStream_t s) {
  using TR = pdsp::FftTraits<LOG2M>;
  const long long ngroups = (batch + TR::ROWS - 1) / TR::ROWS;
  const dim3 block(TR::WG);
  auto launch = [&](auto fast_c, auto win_c) {
    auto go = [&](auto peak_c) {
      hipLaunchKernelGGL((pdsp::spectrum_packed_kernel<T, LOG2M, fast_c, win_c, peak_c>), dim3((unsigned)ngroups), block,
                         0, s, frames, win, wf, frame_len, stride, tw, twr, amp, ph, two_sided, s_edge, s_mid, peaks,
                         freq_scale, batch);
    };
    if constexpr (sizeof(T) == 4) {
      if (peaks) go(std::true_type{});
      else go(std::false_type{});
    } else {
      go(std::false_type{});  // fused peaks: f32 only
    }
    return hipGetLastError();
  };
  // fused cosine-sum windows (wmode 2 / 3): whole f32 frames of N = 1024 ... 8192 (the sizes whose plans
  // carry the angle-addition tables); everything else reads the window as a table
  if constexpr (sizeof(T) == 4 && LOG2M >= 9 && LOG2M <= 12) {
    if (fast && wmode == 2) return launch(std::true_type{}, int_c<2>{});
    if (fast && wmode == 3) return launch(std::true_type{}, int_c<3>{});
  }
  if (fast && win) return launch(std::true_type{}, int_c<1>{});
  if (fast) return launch(std::true_type{}, int_c<0>{});
  if (win) return launch(std::false_type{}, int_c<1>{});
  return launch(std::false_type{}, int_c<0>{});
}

template <typename T, class... A>
hipError_t launch_packed(int log2m, A... a) {
  return with_int<5, 13>(log2m, hipErrorInvalidValue, [&](auto L) { return launch_packed_one<T, L>(a...); });
}

template <typename T>
hipError_t launch_real(int log2m, const T *x, T *ore, T *oim, T scale, const typename pdsp::vec2<T>::type *tw,
                       const typename pdsp::vec2<T>::type *twr, long long batch, hipStream_t s) {
  return with_int<12, 13>(log2m, hipErrorInvalidValue, [&](auto L) {
    using TR = pdsp::FftTraits<L, 4>;
    hipLaunchKernelGGL((pdsp::fft_real_kernel<T, L>), dim3((unsigned)((batch + TR::ROWS - 1) / TR::ROWS)), dim3(TR::WG),
                       0, s, x, ore, oim, scale, tw, twr, batch);
    return hipGetLastError();
  });
}

// Four-step transform of `batch` rows of N = N1*N2 points into scratch planes (pass A + B);
// the caller runs pass C.  REAL rows may carry a window and be shorter than N.
template <typename T>
int fourstep_ab(const pdsp_plan *plan, const Pick &p, long long batch, const T *re_in, const T *im_in, const T *win,
                long long in_stride, long long frame_len, T *s_re, T *s_im, hipStream_t s) {
  const Tables<T> &t = tables<T>(plan);
  const int n2 = 1 << t.log2n2;
  const long long blocks = batch * (n2 / 256);
  if (int rc = check_grid(blocks, batch)) return rc;
  const TwAB<T> w = twab(t);
  const bool known = with_int<1, 4>(t.log2n1, false, [&](auto L) {
    auto go = [&](auto real_c, auto win_c) {
      hipLaunchKernelGGL((pdsp::fourstep_cols_kernel<T, L, real_c, win_c>), dim3((unsigned)blocks), dim3(256), 0, s,
                         re_in, im_in, win, s_re, s_im, w.a, w.b, n2, in_stride, frame_len, batch);
    };
    if (im_in) go(std::false_type{}, std::false_type{});
    else if (win) go(std::true_type{}, std::true_type{});
    else go(std::true_type{}, std::false_type{});
    return true;
  });
  if (!known) return fail(PDSP_ERR_UNSUPPORTED_SIZE, "unsupported four-step split");
  PDSP_HIP_TRY(hipGetLastError());
  // pass B: the N1 * batch rows of N2 points, in place (each workgroup loads its row before it stores)
  pdsp::LoadComplex<T> ld{s_re, s_im, n2};
  pdsp::StoreComplex<T> st{s_re, s_im, n2, T(1)};
  PDSP_HIP_TRY(launch_rows<T>(p.rows, t, t.log2n2, ld, st, batch << t.log2n1, s));
  return PDSP_OK;
}

template <typename T, int MODE>
int fourstep_c(const pdsp_plan *plan, long long batch, const T *s_re, const T *s_im, T *o1, T *o2, T scale, int bins,
               int nyq, T s_edge, T s_mid, hipStream_t s) {
  const Tables<T> &t = tables<T>(plan);
  const int n2 = 1 << t.log2n2;
  const long long blocks = batch * (n2 / 256);
  const bool known = with_int<1, 4>(t.log2n1, false, [&](auto L) {
    hipLaunchKernelGGL((pdsp::fourstep_out_kernel<T, L, MODE>), dim3((unsigned)blocks), dim3(256), 0, s, s_re, s_im,
                       o1, o2, n2, scale, bins, nyq, s_edge, s_mid, batch);
    return true;
  });
  if (!known) return fail(PDSP_ERR_UNSUPPORTED_SIZE, "unsupported four-step split");
  PDSP_HIP_TRY(hipGetLastError());
  return PDSP_OK;
}

// fft_staged_kernel on planar complex rows of 32 <= N <= 256 points (16-byte aligned planes).
template <typename T>
hipError_t launch_staged_complex(int log2n, const pdsp::LoadComplex<T> &ld, const pdsp::StoreComplex<T> &st,
                                 const typename pdsp::vec2<T>::type *tw, long long rows, hipStream_t s) {
  const long long blocks = ((rows << log2n) + 4095) / 4096;
  return with_int<5, 8>(log2n, hipErrorInvalidValue, [&](auto L) {
    hipLaunchKernelGGL((pdsp::fft_staged_kernel<T, L, pdsp::LoadComplex<T>, pdsp::StoreComplex<T>>),
                       dim3((unsigned)blocks), dim3(256), 0, s, ld, st, tw, rows);
    return hipGetLastError();
  });
}

// findPeak over stored amplitude rows, the tail of every spectrum path: the index array and / or the SpectrumPeak
// records that the spectrum kernel did not write itself (Pick::fused_peaks), on the kernels of Pick::peaks.  Each
// case of spectrum_impl's switch returns through it.
template <typename T>
struct PeakTail {
  const Pick &p;
  int bins;
  T freq_scale;
  int32_t *peak_idx;
  pdsp_peak32 *peaks;
  long long batch;
  hipStream_t s;
  int operator()(const T *amp, const T *ph) const {
    pdsp::PeakRec *recs = p.fused_peaks ? nullptr : reinterpret_cast<pdsp::PeakRec *>(peaks);
    if (p.peaks & kPeakWave)
      hipLaunchKernelGGL((pdsp::peak_wave_kernel<T>), dim3((unsigned)((batch + 3) / 4)), dim3(256), 0, s, amp, ph, bins,
                         freq_scale, peak_idx, recs, batch);
    if (p.peaks & kPeakFind)
      hipLaunchKernelGGL((pdsp::find_peak_kernel<T>), dim3((unsigned)batch), dim3(256), 0, s, amp, bins, peak_idx, batch);
    if (p.peaks & kPeakFromRows)
      hipLaunchKernelGGL((pdsp::peak_from_rows_kernel<T>), dim3((unsigned)batch), dim3(256), 0, s, amp, ph, bins,
                         freq_scale, recs, batch);
    if (p.peaks) PDSP_HIP_TRY(hipGetLastError());
    return PDSP_OK;
  }
};

// fft_tiny_staged_kernel for 2 <= N <= 16 (one thread per row, chunk staged through LDS).
template <typename T, bool AMP, class LD>
hipError_t launch_tiny(int log2n, const LD &ld, const T *win, T *o1, T *o2, T scale, int bins, int nyq, T s_edge,
                       T s_mid, long long batch, hipStream_t s) {
  const long long blocks = ((batch << log2n) + 4095) / 4096;
  // N = 32 transforms have fft_staged_kernel; the spectrum of N = 32 frames comes here
  return with_int<1, AMP ? 5 : 4>(log2n, hipErrorInvalidValue, [&](auto L) {
    hipLaunchKernelGGL((pdsp::fft_tiny_staged_kernel<T, L, AMP, LD>), dim3((unsigned)blocks), dim3(256), 0, s, ld, win,
                       o1, o2, scale, bins, nyq, s_edge, s_mid, batch);
    return hipGetLastError();
  });
}

// General four-step path (log2n1 > kMaxLog2N1), steps 1-4 of bigfft_transpose_kernel's header:
// transposes `in` into (a_re, a_im) = [n2][n1], N1-point rows in place, twiddled transpose into
// (b_re, b_im) = [k1][n2], N2-point rows in place.  Step 5 is bigfft_out.
template <typename T>
int bigfft_rows(const pdsp_plan *plan, const Pick &p, long long batch, const T *re_in, const T *im_in, const T *win,
                long long in_stride, long long used, T *a_re, T *a_im, T *b_re, T *b_im, hipStream_t s) {
  const Tables<T> &t = tables<T>(plan);
  const int n1 = 1 << t.log2n1, n2 = 1 << t.log2n2;
  const long long tiles = batch * (plan->n / 1024);
  if (tiles >= (1LL << 31) || (batch << t.log2n2) >= (1LL << 31))
    return fail(PDSP_ERR_BAD_ARG, "batch %lld is too large for FFT size %lld", batch, plan->n);
  hipLaunchKernelGGL((pdsp::bigfft_transpose_kernel<T, false, false>), dim3((unsigned)tiles), dim3(256), 0, s, re_in,
                     im_in, win, used, in_stride, t.twa, t.twb, a_re, a_im, n1, n2, T(1), 0, 0, T(0), T(0));
  PDSP_HIP_TRY(hipGetLastError());
  {
    pdsp::LoadComplex<T> ld{a_re, a_im, n1};
    pdsp::StoreComplex<T> st{a_re, a_im, n1, T(1)};
    if (p.n1_square) PDSP_HIP_TRY(launch_rows<T>(p.n1_rows, t, t.log2n1, ld, st, batch << t.log2n2, s));
    else if (p.n1_rows == kStaged) PDSP_HIP_TRY(launch_staged_complex<T>(t.log2n1, ld, st, t.tw1, batch << t.log2n2, s));
    else PDSP_HIP_TRY(launch_fft<T>(t.log2n1, ld, st, t.tw1, batch << t.log2n2, s));
  }
  hipLaunchKernelGGL((pdsp::bigfft_transpose_kernel<T, true, false>), dim3((unsigned)tiles), dim3(256), 0, s, a_re, a_im,
                     (const T *)nullptr, plan->n, plan->n, t.twa, t.twb, b_re, b_im, n2, n1, T(1), 0, 0, T(0), T(0));
  PDSP_HIP_TRY(hipGetLastError());
  pdsp::LoadComplex<T> ld{b_re, b_im, n2};
  pdsp::StoreComplex<T> st{b_re, b_im, n2, T(1)};
  PDSP_HIP_TRY(launch_rows<T>(p.rows, t, t.log2n2, ld, st, batch << t.log2n1, s));
  return PDSP_OK;
}

// Step 5: [k1][k2] -> natural order.  AMP = false: complex planes (o1, o2) times `scale`;
// AMP = true: amplitude rows o1 (and phase rows o2 unless null) of `bins` values.
template <typename T, bool AMP>
int bigfft_out(const pdsp_plan *plan, long long batch, const T *b_re, const T *b_im, T *o1, T *o2, T scale, int bins,
               int nyq, T s_edge, T s_mid, hipStream_t s) {
  const Tables<T> &t = tables<T>(plan);
  const long long tiles = batch * (plan->n / 1024);
  hipLaunchKernelGGL((pdsp::bigfft_transpose_kernel<T, false, AMP>), dim3((unsigned)tiles), dim3(256), 0, s, b_re, b_im,
                     (const T *)nullptr, plan->n, plan->n, t.twa, t.twb, o1, o2, 1 << t.log2n1, 1 << t.log2n2, scale,
                     bins, nyq, s_edge, s_mid);
  PDSP_HIP_TRY(hipGetLastError());
  return PDSP_OK;
}

// One tile pass over a factor of 2^l points on the kernel pick_tiles chose: tile_pass_kernel (tile width by factor:
// 64 / 32 / 32 / 16), or for a 512-point factor the 32-wide tiles of tile_cols512_kernel / tile_rows512_kernel.
// real_in = tile_pass_kernel's IN: 0 complex planes, 1 real rows (in_im unused), 2 real rows times the window table
// in in_im, 3 / 4 the same for packed real rows (two samples per point)
template <typename T, bool COLS>
int tile_pass(int kernel, int l, int real_in, const T *in_re, const T *in_im, T *out_re, T *out_im,
              const typename pdsp::vec2<T>::type *tw, const Tables<T> &t, pdsp::TileGeom g, T scale, long long batch,
              hipStream_t s) {
  const long long blocks = batch * g.nblk * g.tiles;
  if (int rc = check_grid(blocks, batch)) return rc;
  const TwAB<T> w = twab(t);
  if constexpr (COLS && sizeof(T) == 4) {
    if (kernel == kTileCols512) {
      g.tiles /= 2;
      const long long wide = batch * g.nblk * g.tiles;
      if (real_in == 1)
        hipLaunchKernelGGL((pdsp::tile_cols512_kernel<T, 1>), dim3((unsigned)wide), dim3(256), 0, s, in_re, in_im, out_re,
                           out_im, t.tw8, w.a, w.b, g, batch);
      else
        hipLaunchKernelGGL((pdsp::tile_cols512_kernel<T, 0>), dim3((unsigned)wide), dim3(256), 0, s, in_re, in_im, out_re,
                           out_im, t.tw8, w.a, w.b, g, batch);
      PDSP_HIP_TRY(hipGetLastError());
      return PDSP_OK;
    }
  }
  if constexpr (!COLS && sizeof(T) == 4) {
    if (kernel == kTileRows512) {
      g.tiles /= 2;
      const long long wide = batch * g.tiles;
      hipLaunchKernelGGL((pdsp::tile_rows512_kernel<T>), dim3((unsigned)wide), dim3(256), 0, s, in_re, in_im, out_re, out_im,
                         t.tw8, w.a, w.b, g, scale, batch);
      PDSP_HIP_TRY(hipGetLastError());
      return PDSP_OK;
    }
  }
  const bool known = with_int<6, 9>(l, false, [&](auto L) {
    auto go = [&](auto in_c) {
      // IN = 0 for row passes; f64 has no fused-window first pass (IN 5 / 6)
      constexpr int IN = (COLS && (in_c < 5 || sizeof(T) == 4)) ? in_c : 0;
      hipLaunchKernelGGL((pdsp::tile_pass_kernel<T, L, tile_width(L), COLS, IN>), dim3((unsigned)blocks), dim3(256), 0,
                         s, in_re, in_im, out_re, out_im, tw, w.a, w.b, g, scale, batch);
      return true;
    };
    return COLS && real_in >= 1 && real_in <= 6 ? with_int<1, 6>(real_in, false, go) : go(int_c<0>{});
  });
  if (!known) return fail(PDSP_ERR_UNSUPPORTED_SIZE, "unsupported tile-pass factor 2^%d", l);
  PDSP_HIP_TRY(hipGetLastError());
  return PDSP_OK;
}

// The pass chain on one set of factor tables: `n` points per transform, p.np factors 2^l[i] with radix tables tw[i],
// each on the kernel p.tile[i]; tshift = 1 when t.twa / t.twb belong to the 2n-point plan.  `first` =
// tile_pass_kernel's IN for the first pass (im_in then carries the window table or nothing); in_batch = distance
// between input rows (real samples for first >= 1).  Every pass reads one plane pair and writes another, so input and
// output may alias each other: two passes go through s1, three through s1 and s2.
template <typename T>
int tilepass_chain(const Tables<T> &t, const Pick &p, long long n, const int *l, typename pdsp::vec2<T>::type *const *tw,
                   unsigned tshift, int first, long long batch, const T *re_in, const T *im_in, long long in_batch,
                   T *re_out, T *im_out, T scale, T *s1_re, T *s1_im, T *s2_re, T *s2_im, hipStream_t s,
                   const pdsp::TileGeom *fused_win = nullptr) {
  auto with_window = [&](pdsp::TileGeom &g) {  // first = 5 / 6: the angle-addition tables and coefficients
    if (fused_win) {
      g.wa = fused_win->wa, g.wb = fused_win->wb, g.wstep = fused_win->wstep, g.we = fused_win->we;
      g.k0 = fused_win->k0, g.k1 = fused_win->k1, g.k2 = fused_win->k2;
    }
  };
  if (p.np == 2) {
    const long long a = 1LL << l[0], b = 1LL << l[1];
    pdsp::TileGeom g1{n, 1, (int)(b / tile_width(l[0])), 0, 0, b, b, 1u, in_batch, tshift};
    with_window(g1);
    if (int rc = tile_pass<T, true>(p.tile[0], l[0], first, re_in, im_in, s1_re, s1_im, tw[0], t, g1, T(1), batch, s))
      return rc;
    pdsp::TileGeom g2{n, 1, (int)(a / tile_width(l[1])), 0, 0, 0, a, 1u, n, tshift};
    return tile_pass<T, false>(p.tile[1], l[1], 0, (const T *)s1_re, (const T *)s1_im, re_out, im_out, tw[1], t, g2, scale,
                               batch, s);
  }
  const long long a = 1LL << l[0], b = 1LL << l[1], c = 1LL << l[2];
  pdsp::TileGeom g1{n, 1, (int)(b * c / tile_width(l[0])), 0, 0, b * c, b * c, 1u, in_batch, tshift};
  with_window(g1);
  pdsp::TileGeom g2{n, (int)a, (int)(c / tile_width(l[1])), b * c, c, c, a * c, (unsigned)a, n, tshift};
  if (p.tile_major) {
    // log2 of the second pass's tile width (512-point columns: 32 on tile_cols512_kernel, 16 on tile_pass_kernel)
    const int lt = l[1] == 6 ? 6 : ((l[1] == 9 && p.tile[1] == kTilePlain) ? 4 : 5);
    g1.perm_lc = l[2], g1.perm_lt = lt, g1.perm_b = (int)b;
    g2.in_tile = b << lt, g2.in_stride = 1LL << lt;
  }
  if (int rc = tile_pass<T, true>(p.tile[0], l[0], first, re_in, im_in, s1_re, s1_im, tw[0], t, g1, T(1), batch, s))
    return rc;
  if (int rc = tile_pass<T, true>(p.tile[1], l[1], 0, (const T *)s1_re, (const T *)s1_im, s2_re, s2_im, tw[1], t, g2, T(1),
                                  batch, s))
    return rc;
  pdsp::TileGeom g3{n, 1, (int)(a * b / tile_width(l[2])), 0, 0, 0, a * b, 1u, n, tshift};
  return tile_pass<T, false>(p.tile[2], l[2], 0, (const T *)s2_re, (const T *)s2_im, re_out, im_out, tw[2], t, g3, scale,
                             batch, s);
}

// The intermediate planes of a multi-pass transform whose last pass cannot run in place (three tile passes, general
// four-step), in p.pairs pairs of drawn scratch `sc`: the pair the last pass reads is drawn; the pair before it is the
// output planes (p.out_first), or where those share bytes with the input a second drawn pair.
template <typename T>
struct Intermediates {
  T *first_re, *first_im, *last_re, *last_im;
};
template <typename T>
Intermediates<T> intermediates(const Pick &p, T *sc, size_t plane, T *re_out, T *im_out) {
  if (p.out_first) return {re_out, im_out, sc, sc + plane};
  if (p.pairs > 1) return {sc + 2 * plane, sc + 3 * plane, sc, sc + plane};
  return {nullptr, nullptr, sc, sc + plane};  // two tile passes: the drawn pair is the only intermediate
}

// The argument checks of run_complex, shared with transform_path (batch == 0 passes: nothing to do)
// Aliasing (DESIGN.md 4.1d has the reasoning kernel by kernel).  Every single-pass kernel gives a workgroup the same
// rows on its input and output sides and loads them whole before its first store, but no workgroup waits for
// another: an output plane may share bytes with an input plane only where the two begin at the same address -- in
// place, exchanged (re_out == im_in, im_out == re_in) or one plane of either.  Shifted by an element, a row or half
// a plane, one workgroup's stores race another's loads.  The multi-pass sizes read the input in a first pass of its
// own (pick_transform draws the scratch for that) and take any overlap.  A size is single-pass by the plan and the
// call's kind alone, never by alignment, batch or a switch: f64 real rows of N = 16384 count as single-pass at every
// batch, because fft_real_kernel runs them from 8 rows on.  Output planes that overlap each other race at every size.
template <typename T>
int check_transform(const pdsp_plan *plan, long long batch, const T *re_in, const T *im_in, const T *re_out,
                    const T *im_out) {
  if (int rc = check_plan_batch(plan, batch)) return rc;
  if (batch == 0) return PDSP_OK;
  if (!re_in || !re_out || !im_out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const Tables<T> &t = tables<T>(plan);
  if (!t.tw)
    return fail(PDSP_ERR_UNSUPPORTED_SIZE, "FFT size %lld exceeds the %d-bit limit %d", plan->n, (int)(8 * sizeof(T)),
                pdsp_max_size((int)sizeof(T)));
  const size_t bytes = (size_t)batch * (size_t)plan->n * sizeof(T);
  if (t.log2n1 <= 0 || (sizeof(T) == 8 && !im_in && plan->log2n == 14)) {
    auto clash = [&](const T *out, const T *in) {  // the disjoint call leaves at the first comparison
      return host_ranges_overlap(out, bytes, in, bytes) && !exact_in_place(out, plan->n, in, plan->n);
    };
    if (clash(re_out, re_in) || clash(im_out, re_in) || clash(re_out, im_in) || clash(im_out, im_in))
      return fail(PDSP_ERR_BAD_ARG, "output overlaps input (an output plane may share bytes with an input plane only "
                                    "where the two begin at the same address)");
  }
  if (host_ranges_overlap(re_out, bytes, im_out, bytes))
    return fail(PDSP_ERR_BAD_ARG, "the output planes overlap each other");
  return PDSP_OK;
}

// pdsp_dev_transform_path_*: the checks and the pick of run_complex, and nothing else
template <typename T>
int transform_path(const pdsp_plan *plan, long long batch, const T *re_in, const T *im_in, const T *re_out,
                   const T *im_out, int *info) {
  if (int rc = check_transform<T>(plan, batch, re_in, im_in, re_out, im_out)) return rc;
  if (!info) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const Pick p = batch ? pick_transform<T>(plan, batch, re_in, im_in, re_out, im_out) : Pick{};
  std::memcpy(info, &p, sizeof(p));
  return PDSP_OK;
}

template <typename T>
int run_complex(const pdsp_plan *plan, long long batch, const T *re_in, const T *im_in, T *re_out, T *im_out, T scale,
                hipStream_t s, bool by_size) {
  if (int rc = check_transform<T>(plan, batch, re_in, im_in, re_out, im_out)) return rc;
  if (batch == 0) return PDSP_OK;
  const Pick p = pick_transform<T>(plan, batch, re_in, im_in, re_out, im_out, by_size);
  const Tables<T> &t = tables<T>(plan);
  DeviceGuard g(plan->device);
  PDSP_HIP_TRY(g.err);
  const size_t plane = (size_t)batch * (size_t)plan->n;
  StreamScratch mem(s);
  if (p.pairs) PDSP_HIP_TRY(mem.alloc((size_t)p.pairs * 2 * plane * sizeof(T)));
  T *const sc = (T *)mem.p;
  const pdsp::StoreComplex<T> st{re_out, im_out, plan->n, scale};
  switch (p.path) {
    case kRealPacked:
      if constexpr (sizeof(T) == 8)
        PDSP_HIP_TRY(launch_real<T>(plan->log2n - 1, re_in, re_out, im_out, scale, t.tw_half, t.twr, batch, s));
      return PDSP_OK;
    case kPaired:
      if constexpr (sizeof(T) == 4) {
        const int lp = plan->log2n - 14;
        const long long blocks = ((batch + 7) / 8) * 8 * (1LL << lp);
        if (int rc = check_grid(blocks, batch)) return rc;
        const TwAB<T> w = twab(t);
        auto paired = [&](auto lp_c) {
          auto go = [&](auto real_c) {
            hipLaunchKernelGGL((pdsp::fft_paired_kernel<T, lp_c, real_c>), dim3((unsigned)blocks), dim3(256), 0, s,
                               re_in, im_in, re_out, im_out, t.tw12, t.tws4, w.a, w.b, scale, batch, pdsp::PairedPacked{});
          };
          if (im_in) go(std::false_type{});
          else go(std::true_type{});
        };
        if (lp == 1) paired(int_c<1>{});
        else paired(int_c<2>{});
        PDSP_HIP_TRY(hipGetLastError());
      }
      return PDSP_OK;
    case kTilePasses:
      if constexpr (sizeof(T) == 4) {
        const Intermediates<T> m = intermediates(p, sc, plane, re_out, im_out);
        const bool two = p.np == 2;  // one intermediate pair: the drawn one
        return tilepass_chain<T>(t, p, plan->n, t.tp_l, t.tp_tw, 0u, im_in ? 0 : 1, batch, re_in, im_in, plan->n, re_out,
                                 im_out, scale, two ? m.last_re : m.first_re, two ? m.last_im : m.first_im,
                                 two ? nullptr : m.last_re, two ? nullptr : m.last_im, s);
      }
      return PDSP_OK;
    case kFourstepGeneral: {
      const Intermediates<T> m = intermediates(p, sc, plane, re_out, im_out);
      int rc = bigfft_rows<T>(plan, p, batch, re_in, im_in, nullptr, plan->n, plan->n, m.first_re, m.first_im, m.last_re,
                              m.last_im, s);
      if (!rc) rc = bigfft_out<T, false>(plan, batch, m.last_re, m.last_im, re_out, im_out, scale, 0, 0, T(0), T(0), s);
      return rc;
    }
    case kFourstepFused: {
      int rc = fourstep_ab<T>(plan, p, batch, re_in, im_in, nullptr, plan->n, plan->n, sc, sc + plane, s);
      if (!rc) rc = fourstep_c<T, 0>(plan, batch, sc, sc + plane, re_out, im_out, scale, 0, 0, T(0), T(0), s);
      return rc;
    }
    case kTinyStaged:  // 2 <= N <= 16: one thread per row
      if (im_in)
        PDSP_HIP_TRY((launch_tiny<T, false>(plan->log2n, pdsp::LoadComplex<T>{re_in, im_in, plan->n}, (const T *)nullptr,
                                            re_out, im_out, scale, 0, 0, T(0), T(0), batch, s)));
      else
        PDSP_HIP_TRY((launch_tiny<T, false>(plan->log2n, pdsp::LoadReal<T>{re_in, plan->n}, (const T *)nullptr, re_out,
                                            im_out, scale, 0, 0, T(0), T(0), batch, s)));
      return PDSP_OK;
    case kStaged: {  // coalesced 16-byte I/O staged through LDS (fft_staged_kernel)
      const long long blocks = (batch * plan->n + 4095) / 4096;
      auto staged = [&](auto L, const auto &ld) {
        using LD = std::decay_t<decltype(ld)>;
        hipLaunchKernelGGL((pdsp::fft_staged_kernel<T, L, LD, pdsp::StoreComplex<T>>), dim3((unsigned)blocks), dim3(256),
                           0, s, ld, st, t.tw, batch);
        return true;
      };
      // (the sizes 5 ... 8 are built for both types; f64 stops at 7: pick_transform)
      with_int<5, 8>(plan->log2n, false, [&](auto L) {
        if (im_in) return staged(L, pdsp::LoadComplex<T>{re_in, im_in, plan->n});
        return staged(L, pdsp::LoadReal<T>{re_in, plan->n});
      });
      PDSP_HIP_TRY(hipGetLastError());
      return PDSP_OK;
    }
    default:  // kStockham / kSplit2 / kSplit4
      if (im_in)
        PDSP_HIP_TRY(launch_rows<T>(p.rows, t, plan->log2n, pdsp::LoadComplex<T>{re_in, im_in, plan->n}, st, batch, s));
      else PDSP_HIP_TRY(launch_rows<T>(p.rows, t, plan->log2n, pdsp::LoadReal<T>{re_in, plan->n}, st, batch, s));
      return PDSP_OK;
  }
}

// Interleaved complex rows (single-pass sizes): forward, or inverse = conj . forward . conj with 1/N.
template <typename T>
int run_interleaved(const pdsp_plan *plan, long long batch, const T *in, T *out, bool inverse, hipStream_t s) {
  if (int rc = check_plan_batch(plan, batch)) return rc;
  if (batch == 0) return PDSP_OK;
  if (!in || !out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (!aligned(2 * sizeof(T), in, out))
    return fail(PDSP_ERR_BAD_ARG, "interleaved rows must be aligned to one (re, im) pair");
  const Tables<T> &t = tables<T>(plan);
  if (!t.tw || t.log2n1 > 0)
    return fail(PDSP_ERR_UNSUPPORTED_SIZE, "interleaved rows are single-pass only: FFT size %lld exceeds %d", plan->n,
                1 << max_log2n<T>());
  // fft_stockham_kernel loads a workgroup's rows whole before it stores them and waits for no other workgroup: the
  // same rows, or no byte in common
  if (const size_t bytes = (size_t)batch * (size_t)plan->n * 2 * sizeof(T);
      host_ranges_overlap(out, bytes, in, bytes) && !exact_in_place(out, plan->n, in, plan->n))
    return fail(PDSP_ERR_BAD_ARG, "output overlaps input (only out == in may share bytes)");
  DeviceGuard g(plan->device);
  PDSP_HIP_TRY(g.err);
  const pdsp::cx<T> *zin = reinterpret_cast<const pdsp::cx<T> *>(in);
  pdsp::cx<T> *zout = reinterpret_cast<pdsp::cx<T> *>(out);
  if (inverse) {
    pdsp::LoadInterleaved<T, true> ld{zin, plan->n};
    pdsp::StoreInterleaved<T, true> st{zout, plan->n, T(1) / (T)plan->n};
    PDSP_HIP_TRY(launch_fft<T>(plan->log2n, ld, st, t.tw, batch, s));
  } else {
    pdsp::LoadInterleaved<T, false> ld{zin, plan->n};
    pdsp::StoreInterleaved<T, false> st{zout, plan->n, T(1)};
    PDSP_HIP_TRY(launch_fft<T>(plan->log2n, ld, st, t.tw, batch, s));
  }
  return PDSP_OK;
}

template <int OP>
int launch_complex_op(long long count, const float *are, const float *aim, const float *bre, const float *bim,
                      long long b_len, float sre, float sim, float *ore, float *oim, hipStream_t s) {
  if (complex_op_vec4(OP <= pdsp::kDiv, count, are, aim, bre, bim, b_len, ore, oim))
    hipLaunchKernelGGL((pdsp::complex_op_kernel<float, OP, 4>), dim3(grid_for(count / 4)), dim3(256), 0, s, are, aim,
                       bre, bim, sre, sim, ore, oim, count, b_len);
  else
    hipLaunchKernelGGL((pdsp::complex_op_kernel<float, OP, 1>), dim3(grid_for(count)), dim3(256), 0, s, are, aim, bre,
                       bim, sre, sim, ore, oim, count, b_len);
  PDSP_HIP_TRY(hipGetLastError());
  return PDSP_OK;
}

// The argument checks of spectrum_impl, shared with spectrum_path (batch == 0 passes: nothing to do)
template <typename T>
int check_spectrum(const pdsp_plan *plan, long long batch, const T *frames, long long frame_len, long long frame_stride,
                   const T *window, int sides, const T *amp_out, const T *phase_out, const int32_t *peak_idx_out,
                   const pdsp_peak32 *peaks_out, double sample_rate) {
  if (int rc = check_plan_batch(plan, batch)) return rc;
  if (sides != PDSP_SIDES_ONE && sides != PDSP_SIDES_TWO) return fail(PDSP_ERR_BAD_ARG, "bad sides %d", sides);
  // frame_stride < frame_len = overlapping frames of one signal (an STFT with hop = frame_stride): rows are only read
  if (frame_len < 0 || frame_stride < 1) return fail(PDSP_ERR_BAD_ARG, "bad frame_len/frame_stride");
  if (peaks_out && sample_rate <= 0)
    return fail(PDSP_ERR_SAMPLE_RATE, "Sample rate must be positive, got %.17g", sample_rate);
  if (batch == 0) return PDSP_OK;
  if (!frames || (!amp_out && !peaks_out)) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if ((phase_out || peak_idx_out) && !amp_out) return fail(PDSP_ERR_BAD_ARG, "phase/peak index output needs amp_out");
  const Tables<T> &t = tables<T>(plan);
  if (!t.tw && !t.tw_half)
    return fail(PDSP_ERR_UNSUPPORTED_SIZE, "FFT size %lld exceeds the %d-bit limit %d", plan->n, (int)(8 * sizeof(T)),
                pdsp_max_size((int)sizeof(T)));
  // a frame with samples on the complex kernel of (x, 0): N < 64, the sizes without packed-real tables
  if (frame_len > 0 && !t.tw_half && t.log2n1 <= 0 && (!t.tw || plan->log2n > 5))
    return fail(PDSP_ERR_UNSUPPORTED_SIZE, "no spectrum tables for size %lld", plan->n);
  // Aliasing: a frame's samples become bins of another length in another order, frames may overlap each other
  // (frame_stride < frame_len), and the peak kernels read the amplitude and phase rows back: no output shares a byte
  // with the frames' extent, with the window's N values or with another output, at any size (DESIGN.md 4.1d).
  const long long n = plan->n, bins = sides == PDSP_SIDES_ONE ? n / 2 + 1 : n, used = frame_len < n ? frame_len : n;
  long long in_count = 0;
  if (used > 0 && (!mad_ok(batch - 1, frame_stride, used, &in_count) || in_count > (LLONG_MAX / 8)))
    return fail(PDSP_ERR_BAD_ARG, "batch %lld x stride overflows", batch);
  const size_t ib = (size_t)in_count * sizeof(T), wb = (size_t)n * sizeof(T), rb = (size_t)batch * (size_t)bins * sizeof(T);
  const void *const out[4] = {amp_out, phase_out, peak_idx_out, peaks_out};
  const size_t ob[4] = {rb, rb, (size_t)batch * sizeof(int32_t), (size_t)batch * sizeof(pdsp_peak32)};
  for (int i = 0; i < 4; ++i) {
    if (host_ranges_overlap(out[i], ob[i], frames, ib) || host_ranges_overlap(out[i], ob[i], window, wb))
      return fail(PDSP_ERR_BAD_ARG, "output overlaps input (the spectrum has no in-place form)");
    for (int j = 0; j < i; ++j)
      if (host_ranges_overlap(out[i], ob[i], out[j], ob[j]))
        return fail(PDSP_ERR_BAD_ARG, "the outputs overlap each other");
  }
  return PDSP_OK;
}

// pdsp_dev_spectrum_path_*: the checks and the pick of spectrum_impl, and nothing else
template <typename T>
int spectrum_path(const pdsp_plan *plan, long long batch, const T *frames, long long frame_len, long long frame_stride,
                  const T *window, int sides, const T *amp_out, const T *phase_out, const int32_t *peak_idx_out,
                  const pdsp_peak32 *peaks_out, double sample_rate, int *info) {
  if (int rc = check_spectrum<T>(plan, batch, frames, frame_len, frame_stride, window, sides, amp_out, phase_out, peak_idx_out,
                                 peaks_out, sample_rate))
    return rc;
  if (!info) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const Pick p = batch ? pick_spectrum<T>(plan, frames, frame_len, frame_stride, window, sides, amp_out, phase_out,
                                          peak_idx_out, peaks_out)
                       : Pick{};
  std::memcpy(info, &p, sizeof(p));
  return PDSP_OK;
}

template <typename T>
int spectrum_impl(const pdsp_plan *plan, long long batch, const T *frames, long long frame_len, long long frame_stride,
                  const T *window, int sides, T *amp_out, T *phase_out, int32_t *peak_idx_out, pdsp_peak32 *peaks_out,
                  double sample_rate, hipStream_t stream) {
  if (int rc = check_spectrum<T>(plan, batch, frames, frame_len, frame_stride, window, sides, amp_out, phase_out, peak_idx_out,
                                 peaks_out, sample_rate))
    return rc;
  if (batch == 0) return PDSP_OK;
  const Pick p = pick_spectrum<T>(plan, frames, frame_len, frame_stride, window, sides, amp_out, phase_out, peak_idx_out,
                                  peaks_out);
  const Tables<T> &t = tables<T>(plan);
  DeviceGuard g(plan->device);
  PDSP_HIP_TRY(g.err);
  static_assert(sizeof(pdsp_peak32) == sizeof(pdsp::PeakRec), "peak record layout");
  const long long n = plan->n;
  const int bins = (int)(sides == PDSP_SIDES_ONE ? n / 2 + 1 : n);
  const long long used = frame_len < n ? frame_len : n;
  const T freq_scale = peaks_out ? (T)(sample_rate / (double)n) : T(0);
  const T s_edge = T(1) / (T)n, s_mid = (sides == PDSP_SIDES_ONE ? T(2) : T(1)) / (T)n;
  const int nyq = (sides == PDSP_SIDES_ONE) ? (int)(n / 2) : -1;
  // the coefficients behind wmode 2 / 3 and first 5 / 6
  const CosineSum cs = p.wmode >= 2 || p.first >= 5 ? cosine_sum(window_kind(t, window)) : CosineSum{};
  pdsp::PeakRec *const fused_recs = p.fused_peaks ? reinterpret_cast<pdsp::PeakRec *>(peaks_out) : nullptr;
  // Scratch: the path's plane pairs (N/2 points each on kSpecTiles), then the amplitude / phase rows that the peak
  // kernels read but the caller did not ask for
  T *amp = amp_out, *ph = phase_out;
  const size_t plane = (size_t)batch * (size_t)(p.path == kSpecTiles ? n / 2 : n), rows = (size_t)batch * bins;
  const size_t extra = p.peaks && !p.fused_peaks ? peak_rows_extra(peaks_out, amp, ph, rows) : 0;
  StreamScratch mem(stream);
  if (p.pairs || extra) PDSP_HIP_TRY(mem.alloc(((size_t)p.pairs * 2 * plane + extra) * sizeof(T)));
  T *const sc = (T *)mem.p;
  if (extra) place_peak_rows(peaks_out, amp, ph, sc + (size_t)p.pairs * 2 * plane, rows);
  const PeakTail<T> tail{p, bins, freq_scale, peak_idx_out, peaks_out, batch, stream};
  switch (p.path) {
    case kSpecMemset:
      if (amp_out) PDSP_HIP_TRY(hipMemsetAsync(amp_out, 0, (size_t)batch * bins * sizeof(T), stream));
      if (phase_out) PDSP_HIP_TRY(hipMemsetAsync(phase_out, 0, (size_t)batch * bins * sizeof(T), stream));
      if (peak_idx_out) PDSP_HIP_TRY(hipMemsetAsync(peak_idx_out, 0, (size_t)batch * sizeof(int32_t), stream));
      if (peaks_out) PDSP_HIP_TRY(hipMemsetAsync(peaks_out, 0, (size_t)batch * sizeof(pdsp_peak32), stream));
      return PDSP_OK;
    case kSpecTiles:
      if constexpr (sizeof(T) == 4) {
        const long long m = n / 2;
        // pass chain: frames -> s1 (-> s2) -> Z; two passes: Z = s2; three passes: Z = s1 again
        T *const s1_re = sc, *const s1_im = sc + plane, *const s2_re = sc + 2 * plane, *const s2_im = sc + 3 * plane;
        T *const z_re = t.hp_np == 2 ? s2_re : s1_re, *const z_im = t.hp_np == 2 ? s2_im : s1_im;
        const T *const wtable = p.first == 4 ? window : (const T *)nullptr;
        pdsp::TileGeom fw{};
        if (p.first >= 5) {
          fw.wa = t.hp_win, fw.wb = fw.wa + 2 * t.hp_win_a, fw.wstep = fw.wb + 2 * 512, fw.we = fw.wstep + 2 * 8;
          fw.k0 = cs.k0, fw.k1 = cs.k1, fw.k2 = cs.k2;
        }
        if (p.head == kHeadSplit4) {
          const pdsp::StoreComplex<T> st{z_re, z_im, m, T(1)};
          with_int<0, 3>(p.first - 3, false, [&](auto W) {  // LoadPackedFrames' window mode: first - 3
            using LD = pdsp::LoadPackedFrames<T, W>;
            hipLaunchKernelGGL((pdsp::fft_split4_kernel<T, 12, LD, pdsp::StoreComplex<T>>), dim3((unsigned)batch),
                               dim3(256), 0, stream,
                               LD{frames, window, frame_stride, fw.wb, fw.we + 2 * 8, fw.we, fw.k0, fw.k1, fw.k2}, st,
                               t.tw12, t.tws4, batch);
            return true;
          });
          PDSP_HIP_TRY(hipGetLastError());
        } else if (p.head == kHeadPaired) {
          const long long blocks = ((batch + 7) / 8) * 8 * 2;
          if (int rc = check_grid(blocks, batch)) return rc;
          const pdsp::PairedPacked pk{frame_stride, fw.wb, fw.we + 2 * 8, fw.we, fw.k0, fw.k1, fw.k2};
          const TwAB<T> w = twab(t);
          with_int<1, 4>(p.first - 2, false, [&](auto PK) {  // fft_paired_kernel's packed loader: first - 2
            hipLaunchKernelGGL((pdsp::fft_paired_kernel<T, 1, false, PK>), dim3((unsigned)blocks), dim3(256), 0, stream,
                               frames, wtable, z_re, z_im, t.tw12, t.tws4, w.a, w.b, T(1), batch, pk);
            return true;
          });
          PDSP_HIP_TRY(hipGetLastError());
        } else if (int rc = tilepass_chain<T>(t, p, m, t.hp_l, t.hp_tw, 1u, p.first, batch, frames, wtable, frame_stride,
                                              z_re, z_im, T(1), s1_re, s1_im, s2_re, s2_im, stream,
                                              p.first >= 5 ? &fw : nullptr)) {
          return rc;
        }
        const long long chunks = m / 2048;  // 256 lanes of four pairs each
        if (int rc = check_grid(batch * chunks, batch)) return rc;
        const TwAB<T> w = twab(t);
        hipLaunchKernelGGL((pdsp::split_amp_rows_kernel<T>), dim3((unsigned)(batch * chunks)), dim3(256), 0, stream,
                           (const T *)z_re, (const T *)z_im, amp, ph, w.a, w.b, (int)m, bins, s_edge, s_mid, batch);
        PDSP_HIP_TRY(hipGetLastError());
        return tail(amp, ph);
      }
      return PDSP_OK;
    case kFourstepGeneral:
    case kFourstepFused: {
      int rc;
      if (p.path == kFourstepGeneral) {
        rc = bigfft_rows<T>(plan, p, batch, frames, nullptr, window, frame_stride, used, sc + 2 * plane, sc + 3 * plane, sc,
                            sc + plane, stream);
        if (!rc) rc = bigfft_out<T, true>(plan, batch, sc, sc + plane, amp, ph, T(1), bins, nyq, s_edge, s_mid, stream);
      } else {
        rc = fourstep_ab<T>(plan, p, batch, frames, nullptr, window, frame_stride, used, sc, sc + plane, stream);
        if (!rc) rc = fourstep_c<T, 1>(plan, batch, sc, sc + plane, amp, ph, T(1), bins, nyq, s_edge, s_mid, stream);
      }
      return rc ? rc : tail(amp, ph);
    }
    case kSpecStaged: {  // (built for f64 too, never picked there: pick_spectrum)
      const long long blocks = (batch * (n / 2) + 4095) / 4096;
      with_int<5, 8>(plan->log2n - 1, false, [&](auto LM) {
        auto go = [&](auto win_c) {
          hipLaunchKernelGGL((pdsp::spectrum_staged_kernel<T, LM, win_c>), dim3((unsigned)blocks), dim3(256), 0, stream,
                             frames, window, t.tw_half, t.twr, amp_out, s_edge, s_mid, batch);
        };
        if (p.wmode) go(std::true_type{});
        else go(std::false_type{});
        return true;
      });
      PDSP_HIP_TRY(hipGetLastError());
      return PDSP_OK;
    }
    case kSpecDif16k:
    case kSpecPacked: {
      // wmode 2 / 3: the kernels take the fused coefficients pre-scaled by s_mid / 2 (a power of two: exact)
      pdsp::WinFused wf{nullptr, nullptr, 0.f, 0.f, 0.f, 1.f};
      if constexpr (sizeof(T) == 4) {
        const float sg = 0.5f * (float)s_mid;
        wf.base = t.wf_base, wf.step = t.wf_step;
        if (cs.terms) wf.k0 = cs.k0 * sg, wf.k1 = cs.k1 * sg, wf.k2 = cs.k2 * sg, wf.edge_ratio = (float)(s_edge / s_mid);
        if (p.path == kSpecDif16k) {
          with_int<0, 3>(p.wmode, false, [&](auto W) {
            auto go = [&](auto peak_c) {
              hipLaunchKernelGGL((pdsp::spectrum_dif16k_kernel<T, W, peak_c>), dim3((unsigned)batch), dim3(256), 0,
                                 stream, frames, window, wf, frame_stride, t.tw12, t.twr, amp_out, s_edge, s_mid,
                                 fused_recs, freq_scale, batch);
            };
            if (fused_recs) go(std::true_type{});
            else go(std::false_type{});
            return true;
          });
          PDSP_HIP_TRY(hipGetLastError());
          return tail(amp, ph);
        }
      }
      PDSP_HIP_TRY(launch_packed<T>(plan->log2n - 1, (bool)p.fast, frames, p.wmode == 0 ? (const T *)nullptr : window,
                                    p.wmode, wf, used, frame_stride, t.tw_half, t.twr, amp_out, phase_out,
                                    sides == PDSP_SIDES_TWO ? 1 : 0, s_edge, s_mid, fused_recs, freq_scale, batch, stream));
      return tail(amp, ph);
    }
    case kSpecTiny:
      PDSP_HIP_TRY((launch_tiny<T, true>(plan->log2n, pdsp::LoadReal<T>{frames, n}, window, amp_out, (T *)nullptr, T(1),
                                         bins, nyq, s_edge, s_mid, batch, stream)));
      return tail(amp, ph);
    default: {  // kSpecSmall
      pdsp::StoreAmplitude<T> st{amp, ph, bins,
                                 // scaleAmplitudeOneSided: `nyquist = size % 2 === 0 ? size/2 : -1`; N = 1 is odd
                                 (sides == PDSP_SIDES_ONE && n % 2 == 0) ? (int)(n / 2) : -1, s_edge, s_mid};
      if (window) {
        pdsp::LoadFrameWindowed<T, true> ld{frames, window, used, frame_stride};
        PDSP_HIP_TRY(launch_fft_small<T>(plan->log2n, ld, st, t.tw, batch, stream));
      } else {
        pdsp::LoadFrameWindowed<T, false> ld{frames, window, used, frame_stride};
        PDSP_HIP_TRY(launch_fft_small<T>(plan->log2n, ld, st, t.tw, batch, stream));
      }
      return tail(amp, ph);
    }
  }
}

template <typename T>
int apply_window_dev(long long batch, long long n, const T *in, const T *window, T *out, hipStream_t s) {
  const long long total = batch * n;
  if (total == 0) return PDSP_OK;
  if (!in || !window || !out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  hipLaunchKernelGGL((pdsp::apply_window_kernel<T>), dim3(grid_for(total)), dim3(256), 0, s, in, window, out, total, n);
  PDSP_HIP_TRY(hipGetLastError());
  return PDSP_OK;
}

template <typename T, bool PHASE>
int polar_dev(long long count, const T *re, const T *im, T *out, hipStream_t s) {
  if (count < 0) return fail(PDSP_ERR_BAD_ARG, "negative size");
  if (count == 0) return PDSP_OK;
  if (!re || !im || !out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  hipLaunchKernelGGL((pdsp::polar_kernel<T, PHASE>), dim3(grid_for(count)), dim3(256), 0, s, re, im, out, count);
  PDSP_HIP_TRY(hipGetLastError());
  return PDSP_OK;
}

inline int complex_op_f32_switch(int op, long long count, const float *a_re, const float *a_im, const float *b_re,
                                 const float *b_im, long long b_len, float sr, float si, float *out_re, float *out_im,
                                 hipStream_t s) {
  switch (op) {
    case PDSP_CX_ADD: return launch_complex_op<pdsp::kAdd>(count, a_re, a_im, b_re, b_im, b_len, sr, si, out_re, out_im, s);
    case PDSP_CX_SUB: return launch_complex_op<pdsp::kSub>(count, a_re, a_im, b_re, b_im, b_len, sr, si, out_re, out_im, s);
    case PDSP_CX_MUL: return launch_complex_op<pdsp::kMul>(count, a_re, a_im, b_re, b_im, b_len, sr, si, out_re, out_im, s);
    case PDSP_CX_DIV: return launch_complex_op<pdsp::kDiv>(count, a_re, a_im, b_re, b_im, b_len, sr, si, out_re, out_im, s);
    case PDSP_CX_CONJ: return launch_complex_op<pdsp::kConj>(count, a_re, a_im, b_re, b_im, b_len, sr, si, out_re, out_im, s);
    case PDSP_CX_SCALE: return launch_complex_op<pdsp::kScale>(count, a_re, a_im, b_re, b_im, b_len, sr, si, out_re, out_im, s);
    default: return launch_complex_op<pdsp::kMulScalar>(count, a_re, a_im, b_re, b_im, b_len, sr, si, out_re, out_im, s);
  }
}

}  // namespace pdsp_host

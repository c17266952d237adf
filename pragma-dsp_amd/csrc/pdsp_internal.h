// pdsp_internal.h -- what the translation units of libpdsp_hip.so share: the plan object and its device tables,
// error reporting, the stream-ordered scratch pool, the development switches, and the DECLARATIONS of the kernel
// dispatchers.  This header is the contract between the two kinds of translation unit the library is built from, cut
// so that (i) the kernels compile in parallel and (ii) a change to the host side of the boundary (the pdsp_capi*.hip
// units: validation, plan tables, caches, staging, the chunked host calls, the extern "C" entry points -- no kernel
// is instantiated there) does not recompile them.  The host units, which share pdsp_host.h (no kernel unit includes
// it), mirror the kernel units family by family:
//   pdsp_capi.hip                 the core: error state, scratch pools, plans and the plan cache, windows, planes,
//                                 the device-pointer transforms, spectra and element-wise entry points; it defines
//                                 what pdsp_host.h declares
//   pdsp_capi_host.hip            the f64 drop-in: the chunked host calls of transforms and spectra
//   pdsp_capi_fir.hip, _stft, _dct, _hilbert, _resample, _chirp (DFT and CZT), _dwt, _ntt, _sdft, _fft2d
//                                 one family each: validators, handle, entry points, host form, switches and queries
// The kernel units:
//   pdsp_kernels_f32_fft.hip      run_complex<float>, run_interleaved<float>, element-wise f32 kernels
//   pdsp_kernels_f32_spectrum.hip spectrum_impl<float> (fused spectrum kernels, findPeak kernels)
//   pdsp_kernels_f64.hip          every dispatcher for double
//   pdsp_kernels_fir.hip          FIR filtering (fused overlap-save) and the filter spectrum, f32 and f64
//   pdsp_kernels_stft.hip         complex STFT and its overlap-add inverse, f32 and f64
//   pdsp_kernels_dct.hip          DCT-II and DCT-III, f32 and f64
//   pdsp_kernels_hilbert.hip      Hilbert transform, analytic signal, envelope and phase, f32 and f64
//   pdsp_kernels_resample.hip     polyphase rate change (upfirdn / resample_poly), f32 and f64
//   pdsp_kernels_dft.hip          any-length DFT (Bluestein's chirp-z algorithm), f32 and f64
//   pdsp_kernels_dwt.hip          multi-level wavelet transform (wavedec / waverec), f32 and f64
//   pdsp_kernels_czt.hip          chirp-z transform and zoom FFT (czt / zoom_fft), f32 and f64
//   pdsp_kernels_ntt.hip          number-theoretic transform and exact convolution over GF(2^64 - 2^32 + 1)
//   pdsp_kernels_sdft.hip         sliding DFT (chosen bins at every hop), f32 and f64
//   pdsp_kernels_fft2d.hip        2-D transform of images (fft2 / ifft2), f32 and f64
// The dispatchers themselves are pdsp_dispatch.inc (templates on the scalar type), explicitly instantiated there.
// Not part of the boundary: nothing outside pragma-dsp_amd/csrc includes this file.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/pdsp_hip.h"
#include "../../include/pdsp_hip_dev.h"
#include "../../include/pdsp_hip_fft2d.h"
#include "pdsp_fft_core.h"

namespace pdsp_host {

// last error text of the calling thread (pdsp_last_error); defined in pdsp_capi.hip
int fail(int code, const char *fmt, ...);

// development switches (tools / tests): 0 routes N = 16384 spectra to spectrum_packed_kernel<13>,
// and 32 <= N <= 256 transforms to the direct kernel instead of fft_staged_kernel
extern int g_split16k;
extern int g_fused_window;  // pdsp_set_fused_window: plan-owned cosine-sum windows evaluated in the kernel
extern int g_twopass;       // pdsp_set_twopass: 2^15 <= N <= 2^18 f32 transforms in two passes (balanced factors)
extern int g_split8k_f32;  // f32 N = 8192 rows on fft_split2_kernel too (A/B: pdsp_set_split16k bit 1)
extern int g_staged_small;
extern int g_real_packed;  // pdsp_set_real_packed: Radix2Fft.forward rows of 512 <= N <= 16384 on fft_real_kernel


#define PDSP_HIP_TRY(expr)                                                              \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return fail(PDSP_ERR_DEVICE, "HIP error %d (%s) at %s", (int)e_, hipGetErrorString(e_), #expr); \
  } while (0)

// Stream-ordered scratch planes of the multi-pass paths, handed back on every exit path, from a pool of the
// engine's own per device whose release threshold is unlimited: the device's default pool hands its memory back at every synchronisation, so that a
// caller who synchronises between transforms (every host-f64 call does) paid a fresh 1-2 GiB allocation --
// a trip through the kernel driver, observed to stall for 0.5-1 s on a busy host -- on each call.  Here the planes
// of the largest transform seen stay with the engine until pdsp_plan_cache_clear() trims the pools.
hipMemPool_t scratch_pool();   // defined in pdsp_capi.hip
void trim_scratch_pools();

// Bytes of scratch planes this process has drawn from the pools since they were last trimmed: pdsp_plan_destroy()
// hands the pools' unused memory back to the device when a plan that needs scratch (N beyond the single-pass
// limit) goes away and anything was drawn -- otherwise GiBs of HBM stay pinned where the caller's allocator
// (PyTorch's, say) cannot see them, long after the last large transform.
extern std::atomic<unsigned long long> g_scratch_drawn;

// What the library holds right now, counted exactly (pdsp_dev_live_resources): touched where a table, a staging
// buffer or a stream is created or freed and where a cached plan is evicted -- never on a launch path.
struct LiveCounters {
  std::atomic<long long> evictions{0};               // cached plans dropped to make room, since load
  std::atomic<long long> tables{0}, table_bytes{0};  // upload_table minus Tables::release
  std::atomic<long long> host_stage{0}, dev_stage{0};  // plans' pinned / device staging buffers
  std::atomic<long long> streams{0};                 // plans' own streams and slot streams
};
extern LiveCounters g_live;

struct StreamScratch {
  void *p = nullptr;
  hipStream_t s;
  explicit StreamScratch(hipStream_t stream) : s(stream) {}
  StreamScratch(const StreamScratch &) = delete;
  StreamScratch &operator=(const StreamScratch &) = delete;
  hipError_t alloc(size_t bytes) {
    g_scratch_drawn += bytes;
    if (hipMemPool_t pool = scratch_pool()) return hipMallocFromPoolAsync(&p, bytes, pool, s);
    return hipMallocAsync(&p, bytes, s);  // no pool of our own on this device: the default one
  }
  ~StreamScratch() {
    if (p) (void)hipFreeAsync(p, s);
  }
};

struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    err = hipGetDevice(&prev);
    if (err == hipSuccess && dev >= 0 && dev != prev) {
      err = hipSetDevice(dev);
      switched = (err == hipSuccess);
    }
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};

inline int ilog2ll(long long n) {
  int l = 0;
  while ((1LL << l) < n) ++l;
  return l;
}

}  // namespace pdsp_host

// Device tables of one precision.
template <typename T>
struct Tables {
  using T2 = typename pdsp::vec2<T>::type;
  T2 *tw = nullptr;       // inter-pass twiddles of the N-point transform (pdsp_radix.h layout)
  // packed-real spectrum path (N >= 64): radix table of the N/2-point transform and the
  // split twiddles W_N^k, 0 <= k <= N/4
  T2 *tw_half = nullptr;
  T2 *twr = nullptr;
  T2 *tw4n = nullptr;  // DCT post- / pre-twiddles W_4N^k, 0 <= k <= N/2 (same plans as twr)
  T2 *tw12 = nullptr;  // N = 16384 only: radix table of the 4096-point sub-transforms (split kernels)
  T2 *tws4 = nullptr;  // rows of 16384 points (log2n2 == 14): W_16384^k, k < 768 (fft_split4_kernel)
  T2 *tws2 = nullptr;  // rows of 8192 points (log2n2 == 13): W_8192^k, k < 256 (fft_split2_kernel; uses tw12 too)
  T *win[4] = {nullptr, nullptr, nullptr, nullptr};  // createWindow(type, N), built on first use
  // N = 16384, f32: per-thread bases and per-q constants of the fused cosine-sum windows
  // (spectrum_dif16k_kernel, WinFused): cos / sin of f*(2 tid + e) and of f*512 q (+ 8192), f = 2 pi / (N - 1)
  float *wf_base = nullptr;
  float *wf_step = nullptr;
  // four-step path (N beyond the single-pass limit): `tw` then belongs to the N2-point rows,
  // N1 = N / N2, and W_N^m = twa[m >> 9] * twb[m & 511]
  int log2n2 = 0;  // log2 of the transform `tw` serves (== log2 N when single-pass)
  int log2n1 = 0;
  T2 *twa = nullptr;
  T2 *twb = nullptr;
  T2 *tw1 = nullptr;  // general four-step path (log2n1 > kMaxLog2N1): radix table of the N1-point rows
  // tile passes (f32): N = product of tp_np balanced factors 2^tp_l[i] (two for 2^15..2^18, three for
  // 2^19..2^27), radix table of each factor's transform
  int tp_np = 0;
  int tp_l[3] = {0, 0, 0};
  T2 *tp_tw[3] = {nullptr, nullptr, nullptr};
  T2 *tw8 = nullptr;  // radix table of the 256-point transform (tile_rows512_kernel's halves of a 512-point factor)
  // the same for the N/2-point transform of the packed-real spectrum path (2^15 <= N <= 2^27): it runs on
  // this plan's twa / twb with doubled exponents (TileGeom::tshift)
  int hp_np = 0;
  int hp_l[3] = {0, 0, 0};
  T2 *hp_tw[3] = {nullptr, nullptr, nullptr};
  float *hp_win = nullptr;  // angle-addition tables of the fused cosine-sum windows (TileGeom::wa ...): wa | wb | wstep | we | wq
  size_t hp_win_a = 0;      // entries (cos, sin pairs) of wa
  // every device allocation made for this precision, the lazily built win[] entries included (upload_table in
  // pdsp_host.h is the one place that adds to it).  Touched under plan->mu or before the plan is published only.
  std::vector<void *> owned;
  size_t owned_bytes = 0;  // of `owned`, for the live counters
  void release() {
    for (void *p : owned) (void)hipFree(p);
    pdsp_host::g_live.tables -= (long long)owned.size();
    pdsp_host::g_live.table_bytes -= (long long)owned_bytes;
    *this = Tables{};
  }
};

struct pdsp_plan {
  long long n = 0;
  int log2n = 0;
  int device = -1;
  Tables<float> t32;
  Tables<double> t64;  // present when the f64 single-pass kernels take this size
  // host-f64 entry points: one stream + growing staging buffers per plan
  std::mutex mu;
  hipStream_t stream = nullptr;
  void *h_stage = nullptr;  // pinned
  size_t h_bytes = 0;
  void *d_stage = nullptr;
  size_t d_bytes = 0;
  // batched host calls large enough to be cut into chunks (run_chunked): one stream per staging slot
  std::vector<hipStream_t> slot_streams;
};

template <typename T> Tables<T> &tables(pdsp_plan *p);
template <> inline Tables<float> &tables<float>(pdsp_plan *p) { return p->t32; }
template <> inline Tables<double> &tables<double>(pdsp_plan *p) { return p->t64; }
template <typename T> const Tables<T> &tables(const pdsp_plan *p) { return tables<T>(const_cast<pdsp_plan *>(p)); }

// Largest log2 N of the single-pass kernels: (N + N/16) complex values must fit 160 KiB of LDS.
template <typename T> constexpr int max_log2n() { return sizeof(T) == 4 ? pdsp::kMaxLog2N_f32 : pdsp::kMaxLog2N_f64; }

namespace pdsp_host {

// Factors of a three-pass transform of 2^lg points (2^18 < 2^lg <= 2^27): balanced, ascending.  (Tried and
// dropped: a 64-point first factor everywhere -- the widest tiles for the one pass that reads strided -- with
// 512-point factors behind it: 2^22 as 64 * 256 * 256 and 2^24 as 64 * 512 * 512 measured -3 % / +1 % against
// 128 * 128 * 256 and 256^3, the long-frame spectrum -2 ... -5 %: profiles/r02_experiments/sweep_large_factors.log.)
inline void three_factors(int lg, int *l) {
  l[0] = lg / 3, l[1] = (lg - l[0]) / 2, l[2] = lg - l[0] - l[1];
}
constexpr int tile_width(int l) { return l == 6 ? 64 : (l == 9 ? 16 : 32); }

inline int grid_for(long long total) {
  long long b = (total + 255) / 256;
  if (b > 2048) b = 2048;  // grid-stride the rest (256 CUs x 8)
  if (b < 1) b = 1;
  return (int)b;
}

// launch_complex_op's choice between complex_op_kernel<T, OP, 4> (16-byte accesses: every plane the op uses on a
// 16-byte boundary, count and a binary op's b_len multiples of 4) and <T, OP, 1>; pdsp_dev_complex_op_vec4 reports it.
inline bool complex_op_vec4(bool binary, long long count, const void *are, const void *aim, const void *bre,
                            const void *bim, long long b_len, const void *ore, const void *oim) {
  const auto on16 = [](const void *p) { return ((uintptr_t)p & 15) == 0; };
  return on16(are) && on16(aim) && on16(ore) && on16(oim) && count % 4 == 0 &&
         (!binary || (on16(bre) && on16(bim) && b_len % 4 == 0));
}

template <int V>
using int_c = std::integral_constant<int, V>;

// A runtime int as a template argument: returns f(int_c<v>{}) for Lo <= v <= Hi and `outside` otherwise.  Only
// the instances Lo ... Hi are compiled, so the range is the set of kernels built.
template <int Lo, int Hi, class R, class F>
R with_int(int v, R outside, const F &f) {
  if constexpr (Lo <= Hi) {
    if (v == Lo) return f(int_c<Lo>{});
    return with_int<Lo + 1, Hi>(v, outside, f);
  } else {
    return outside;
  }
}

// Workgroups of a packed-real launch (pdsp_packed.h: PackedRow<T, LOG2M>::TR::ROWS rows each, kPackedWG<LOG2M>
// threads) for `rows` rows; the packed sizes are 5 <= log2m <= 13 (N = 64 ... 16384)
template <int LOG2M>
dim3 packed_grid(long long rows) {
  constexpr int R = pdsp::FftTraits<LOG2M>::ROWS;
  return dim3((unsigned)((rows + R - 1) / R));
}

// A launch of `blocks` workgroups for `batch` rows must fit grid.x (2^31 - 1)
inline int check_grid(long long blocks, long long batch) {
  if (blocks > 0x7fffffffLL) return fail(PDSP_ERR_BAD_ARG, "batch too large: %lld", batch);
  return PDSP_OK;
}

inline int check_plan_batch(const pdsp_plan *plan, long long batch) {
  if (!plan) return fail(PDSP_ERR_BAD_ARG, "plan is null");
  if (batch < 0) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 0, got %lld", batch);
  return check_grid(batch, batch);  // one workgroup per row at most; far beyond any HBM-resident batch
}

// Byte ranges, not pointer equality: do [a, a + a_bytes) and [b, b + b_bytes) share a byte?  A null pointer or an empty
// range shares none.  (The argument checks of the pdsp_capi*.hip units and pdsp_dispatch.inc's.)
inline bool host_ranges_overlap(const void *a, size_t a_bytes, const void *b, size_t b_bytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && a_bytes && b_bytes && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// a*b + c without overflow into *out
inline bool mad_ok(long long a, long long b, long long c, long long *out) {
  long long p;
  return !__builtin_mul_overflow(a, b, &p) && !__builtin_add_overflow(p, c, out);
}

// The one overlap of an output with its input that the row kernels with an in-place form allow: the same rows.
inline bool exact_in_place(const void *out, long long out_stride, const void *in, long long in_stride) {
  return out == in && out_stride == in_stride;
}

// ---- kernel dispatchers: defined in pdsp_dispatch.inc, instantiated for float / double in the kernel units -------
// Rows of planar complex points -> rows (forward; the callers swap planes and pass 1/N for the inverse).
// by_size: the kernel variant is chosen from the plan and the call's kind alone, never from `batch` (the host forms,
// whose `batch` is whatever piece of the caller's rows a chunk holds).
template <typename T>
int run_complex(const pdsp_plan *plan, long long batch, const T *re_in, const T *im_in, T *re_out, T *im_out, T scale,
                hipStream_t s, bool by_size = false);
template <typename T>
int run_interleaved(const pdsp_plan *plan, long long batch, const T *in, T *out, bool inverse, hipStream_t s);
// The batched body of spectrum() (pdsp_spectrum_f32 / _f64 / pdsp_spectrum_peaks_f32).
template <typename T>
int spectrum_impl(const pdsp_plan *plan, long long batch, const T *frames, long long frame_len, long long frame_stride,
                  const T *window, int sides, T *amp_out, T *phase_out, int32_t *peak_idx_out, pdsp_peak32 *peaks_out,
                  double sample_rate, hipStream_t stream);
// pdsp_dev_transform_path_* / pdsp_dev_spectrum_path_*: the argument checks and the decision of run_complex /
// spectrum_impl (pdsp_dispatch.inc: Pick) written to info[PDSP_DEV_PATH_INFO]; no HIP call
template <typename T>
int transform_path(const pdsp_plan *plan, long long batch, const T *re_in, const T *im_in, const T *re_out,
                   const T *im_out, int *info);
template <typename T>
int spectrum_path(const pdsp_plan *plan, long long batch, const T *frames, long long frame_len, long long frame_stride,
                  const T *window, int sides, const T *amp_out, const T *phase_out, const int32_t *peak_idx_out,
                  const pdsp_peak32 *peaks_out, double sample_rate, int *info);
template <typename T>
int apply_window_dev(long long batch, long long n, const T *in, const T *window, T *out, hipStream_t s);
template <typename T, bool PHASE>
int polar_dev(long long count, const T *re, const T *im, T *out, hipStream_t s);
// pdsp_complex_op_f32 after validation: op is a pdsp_complex_op
int complex_op_f32(int op, long long count, const float *are, const float *aim, const float *bre, const float *bim,
                   long long b_len, float sre, float sim, float *ore, float *oim, hipStream_t s);

// pdsp_fir_filter_* / pdsp_fir_spectrum_* after validation (pdsp_kernels_fir.hip): p = the taps the kernel runs with
// (ntaps, or ntaps + 1 zero tap for an even hop), nblk = blocks of hop = N - p + 1 outputs per row, len >= 1
template <typename T>
int fir_filter_dev(const pdsp_plan *plan, long long batch, const T *x, long long len, long long x_stride,
                   const T *h_re, const T *h_im, int p, long long y_off, long long y_len, T *y, long long y_stride,
                   long long nblk, hipStream_t s);
template <typename T>
int fir_spectrum_dev(const pdsp_plan *plan, const T *taps, int ntaps, T *h_re, T *h_im, hipStream_t s);

// pdsp_stft_complex_* / pdsp_istft_* after validation (pdsp_kernels_stft.hip): 64 <= N <= 16384, frames >= 1,
// 1 <= frame_len <= N, hop >= 1; window null (rect) or N values
extern int g_istft_chunk_frames;  // pdsp_set_istft_chunk_frames: frames per chunk of the two-pass inverse (0: default)
template <typename T>
int stft_complex_dev(const pdsp_plan *plan, long long batch, const T *frames, long long frame_len,
                     long long frame_stride, const T *window, T *re_out, T *im_out, hipStream_t s);
template <typename T>
int istft_dev(const pdsp_plan *plan, long long frames, const T *re_in, const T *im_in, long long hop, const T *window,
              T *out, hipStream_t s);
// bytes of stream-ordered scratch istft_dev draws (0 when hop >= N)
template <typename T>
size_t istft_scratch_bytes(long long n, long long hop, long long frames);

// pdsp_dct_* after validation (pdsp_kernels_dct.hip): 64 <= N <= 16384, 1 <= batch < 2^31, strides >= N, type 2 or 3;
// every output (type 2) or input (type 3) scaled by g, index 0 by g0 instead.  y == x with y_stride == x_stride is
// allowed (exact in place), no other overlap.
template <typename T>
int dct_dev(const pdsp_plan *plan, long long batch, const T *x, long long x_stride, int type, T g, T g0, T *y,
            long long y_stride, hipStream_t s);
// the 16-byte path's condition: both row pointers 16-byte aligned, both strides multiples of 16 bytes
bool dct_fast_path(const void *x, long long x_stride, const void *y, long long y_stride, size_t elem);

// pdsp_hilbert_* after validation (pdsp_kernels_hilbert.hip): 64 <= N <= 16384, 1 <= batch < 2^31, 1 <= len <= N,
// x_stride >= len, y_stride >= N (ANALYTIC: 2N), out_mode a pdsp_hilbert_out.  y == x with y_stride == x_stride is
// allowed in the three N-out modes (exact in place), no other overlap.
template <typename T>
int hilbert_dev(const pdsp_plan *plan, long long batch, const T *x, long long x_stride, long long len, int out_mode,
                T *y, long long y_stride, hipStream_t s);
// the wide path's condition: len == N, x rows aligned to 2 elements with an even stride, y rows aligned to 2 elements
// (ANALYTIC: to 16 bytes) with a stride that keeps that
bool hilbert_fast_path(const void *x, long long x_stride, long long len, long long n, int out_mode, const void *y,
                       long long y_stride, size_t elem);

// pdsp_upfirdn_* after validation (pdsp_kernels_resample.hip): 1 <= up, down, ntaps <= 8192, 0 <= t0 < ntaps + up,
// len, batch, y_len >= 1, strides >= the row lengths, y_len * down + t0 within 64 bits, no overlap.  g: the phase-major
// tap table, up * ceil(ntaps / up) device values.
template <typename T>
int upfirdn_dev(const T *g, long long up, long long down, long long ntaps, long long t0, long long batch, const T *x,
                long long len, long long x_stride, T *y, long long y_len, long long y_stride, hipStream_t s);
// The tile of one launch (the rule: pdsp_kernels_resample.hip): the instantiation (r outputs per item,
// win: sliding window, gt: taps in global memory), taps per phase and their LDS row stride, outputs per phase and
// tile, samples staged, dynamic LDS, items per tile.  false: nothing fits (not within the supported domain).
struct UpfirdnTile {
  int r = 0;
  bool win = false, gt = false;
  int tn = 0, tp = 0, bper = 0, span = 0;
  size_t lds_bytes = 0;
  long long items = 0;
};
bool upfirdn_tile(long long up, long long down, long long ntaps, long long y_len, size_t elem, UpfirdnTile *out);
// pdsp_set_upfirdn_tile: low 4 bits 0 = the rule, 1 ... 4 = one instantiation forced; the rest a cap on bper (0: none)
extern int g_upfirdn_tile;
// upfirdn_tile, or PDSP_ERR_UNSUPPORTED_SIZE with a message that names a forced instantiation
int upfirdn_tile_checked(long long up, long long down, long long ntaps, long long y_len, size_t elem, UpfirdnTile *out);

// pdsp_dft_c2c_* after validation (pdsp_kernels_dft.hip): 2 <= len <= 4096, M = 2^log2m = max(32, the power of two >=
// 2 len - 1), 1 <= batch < 2^31, strides >= len, im_in null for real rows; chirp: c[n], len entries; bt: FFT_M(b) / M, M
// entries; tw: the radix table of the M-point transform (the tw_half layout).  Exact in place is allowed, no other
// overlap.
template <typename T>
int dft_dev(int log2m, long long len, long long batch, const T *re_in, const T *im_in, long long in_stride, T *re_out,
            T *im_out, long long out_stride, const typename pdsp::vec2<T>::type *chirp,
            const typename pdsp::vec2<T>::type *bt, const typename pdsp::vec2<T>::type *tw, bool inverse,
            hipStream_t s);

// pdsp_dwt_forward_* / pdsp_dwt_inverse_* after validation (pdsp_kernels_dwt.hip): f even, 2 <= f <= 32, levels >= 1,
// len a positive multiple of 2^levels, batch >= 1, strides >= len, batch * t.tiles < 2^31, no overlap (resident: the
// exact in-place call excepted); hg: h | g, 2 f device values; t from dwt_tile_checked for the same call.
struct DwtTile {
  bool resident = false;
  long long tile = 0, halo = 0, tiles = 0;
  size_t lds_bytes = 0;
};
// pdsp_set_dwt_tile: bits 0-1 0 = the rule, 1 = resident, 2 = tiled; the rest a cap on the tile (0: none)
extern int g_dwt_tile;
// The path and tile of one launch (the rule: pdsp_kernels_dwt.hip), or PDSP_ERR_UNSUPPORTED_SIZE
int dwt_tile_checked(long long f, long long levels, long long n, size_t elem, bool inverse, DwtTile *out);
int dwt_tiled_max_levels(long long f, size_t elem);
template <typename T>
int dwt_dev(const DwtTile &t, const T *hg, int f, int levels, bool inverse, long long batch, const T *in, long long len,
            long long in_stride, T *out, long long out_stride, hipStream_t s);

// pdsp_czt_* after validation (pdsp_kernels_czt.hip): len, bins >= 1, len + bins - 1 <= 8192, M = 2^log2m = max(32, the
// power of two >= len + bins - 1), 1 <= batch < 2^31, in_stride >= len, out_stride >= bins, im_in null for real rows;
// pre: a^-n w^(n^2/2), len entries; post: w^(k^2/2), bins entries; bt: FFT_M(b) / M, M entries; tw: the radix table of
// the M-point transform (the tw_half layout).  Exact in place is allowed, no other overlap.
template <typename T>
int czt_dev(int log2m, long long len, long long bins, long long batch, const T *re_in, const T *im_in,
            long long in_stride, T *re_out, T *im_out, long long out_stride, const typename pdsp::vec2<T>::type *pre,
            const typename pdsp::vec2<T>::type *post, const typename pdsp::vec2<T>::type *bt,
            const typename pdsp::vec2<T>::type *tw, hipStream_t s);

// pdsp_ntt_* after validation (pdsp_kernels_ntt.hip): kNttMinLog2N <= log2n <= kNttMaxLog2N, op a pdsp::NttOp (0 forward,
// 1 inverse, 2 convolution), 1 <= batch with at most 2^31 - 1 workgroups, 1 <= a_len, b_len, out_len <= N (transforms:
// a_len = out_len = N, b unused), strides >= the lengths (b_stride 0: one shared row); tw: omega_N^j, j < N / 2.  out == a
// with equal strides is allowed (a thread stores the positions it loaded), no other overlap.
constexpr int kNttMinLog2N = 6, kNttMaxLog2N = 14;
int ntt_dev(int log2n, int op, long long batch, const uint64_t *a, long long a_stride, int a_len, const uint64_t *b,
            long long b_stride, int b_len, uint64_t *out, long long out_stride, int out_len, const uint64_t *tw,
            hipStream_t s);
// workgroups of that launch (rows per workgroup: pdsp_ntt_kernel.h, NttTraits)
long long ntt_blocks(int log2n, int op, long long batch);
// out[i] = a[i] b[i] mod p, i < count, count >= 1
int ntt_mul_dev(long long count, const uint64_t *a, const uint64_t *b, uint64_t *out, hipStream_t s);

// pdsp_sdft_* after validation (pdsp_kernels_sdft.hip): 2 <= n <= 16384, hop >= 1, 1 <= nbins <= 256, ncomp 1, 3 or 5
// with their weights, samples >= n, in_stride >= samples, out_stride >= 1 + (samples - n) / hop, batch >= 1 with
// sdft_blocks() < 2^31, no overlap; tab: per bin and component n + 1 phases (pdsp_sdft_kernel.h).
// E, the positions per thread: the summation order depends on n and the precision through it alone (f64 keeps 4: at 8
// its kernel runs out of scalar registers)
inline int sdft_segment(long long n, size_t elem) { return elem == 4 && n > 1024 ? 8 : 4; }
int sdft_tile_chunks(long long n, size_t elem);
// workgroups of that launch, or -1 where the product overflows
long long sdft_blocks(long long n, size_t elem, long long samples, long long nbins, long long batch);
template <typename T>
int sdft_dev(long long n, long long hop, int nbins, int ncomp, const double *weights, long long batch, const T *in,
             long long in_stride, long long samples, T *re_out, T *im_out, long long out_stride,
             const typename pdsp::vec2<T>::type *tab, hipStream_t s);

// pdsp_fft2d_* after validation (pdsp_kernels_fft2d.hip).  The one decision of the family, shared by the launch code and
// pdsp_fft2d_query: H and W powers of two, 16 <= H <= 512, 16 <= W <= the single-pass row limit of the precision.
//   H*W <= 4096: resident -- one launch, `images` = 4096 / (H*W) whole images per 256-thread workgroup;
//   else two passes -- the W-plan's row kernels, then one column launch on tiles of `tile` adjacent columns of one
//   image: 256 (one thread per column) at H = 16, 32; at H >= 64 segments of at least 128 bytes where W allows it --
//   64 columns at H = 64 and 32 at H = 128 (one round of the workgroup's LDS rows), 32 (f32) / 16 (f64) at H = 256 and
//   512 (the LDS that fits; at H = 512 in f32 32 columns in one workgroup per CU measured 6-12 % ahead of 16 in two:
//   DESIGN.md 4.18, profiles/fft2d_tile512_ab.txt) -- and never wider than W.
#ifndef PDSP_FFT2D_TILE512_F32
#define PDSP_FFT2D_TILE512_F32 32  /* columns per tile at H = 512 in f32: 32 (139,776 B of LDS, one workgroup per CU) or 16 (69,888 B, two); A/B builds: make EXTRA=-DPDSP_FFT2D_TILE512_F32=16 */
#endif
struct Fft2dPath {
  bool resident = false;
  int images = 0, tile = 0, launches = 0;
};
inline bool fft2d_path(long long h, long long w, size_t elem, Fft2dPath *out) {
  const long long wmax = 1LL << (elem == 4 ? pdsp::kMaxLog2N_f32 : pdsp::kMaxLog2N_f64);
  if ((elem != 4 && elem != 8) || h < 16 || h > 512 || w < 16 || w > wmax || (h & (h - 1)) || (w & (w - 1))) return false;
  Fft2dPath p;
  if (h * w <= 4096) {
    p.resident = true, p.images = (int)(4096 / (h * w)), p.launches = 1;
  } else {
    const long long wide = h <= 32 ? 256 : h == 64 ? 64 : h == 128 ? 32 : elem == 8 ? 16 : h == 256 ? 32 : PDSP_FFT2D_TILE512_F32;
    p.tile = (int)(wide < w ? wide : w), p.launches = 2;
  }
  *out = p;
  return true;
}
// plan_w / plan_h: the plans of W and H points on the handle's device (made current by the caller); im_in null: real
// images; forward kernels only (the caller swaps planes for the inverse); scale: the norm's, applied in the last store
template <typename T>
int fft2d_dev(const Fft2dPath &path, const pdsp_plan *plan_w, const pdsp_plan *plan_h, long long batch, const T *re_in,
              const T *im_in, T *re_out, T *im_out, T scale, hipStream_t s);

}  // namespace pdsp_host

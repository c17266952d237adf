/*
 * pdsp_hip_dev.h -- development switches of libpdsp_hip.so.  NOT part of the drop-in boundary: the reference has
 * nothing like them (src/core/fft.ts and src/xform/fourier.ts select no algorithms), a binding of pdsp_hip.h never
 * includes this file, and every default is the production path.  They exist so that the parity tests can run the
 * same input through two kernels of the engine and hold both to the oracle (tests/test_gpu_*.py), and so that
 * the scripts under tools/ can time one against the other inside one process.  Process-wide; each returns the previous value.
 */
#ifndef PDSP_HIP_DEV_H
#define PDSP_HIP_DEV_H

#include "pdsp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Kernel selection switch for A/B tests (process-wide; returns the previous value): 1 (default)
 * runs whole pair-aligned one-sided N = 16384 f32 spectra on spectrum_dif16k_kernel (two 4096-point
 * sub-transforms per workgroup, decimation in frequency on top) and 16-byte aligned N = 16384 f32
 * complex/real rows on fft_split4_kernel (four 4096-point sub-transforms per workgroup), and N = 8192
 * rows (f64; f32 real input) on fft_split2_kernel; 0 on spectrum_packed_kernel<13> and the
 * single-pass fft_stockham_kernel.  Same results within rounding.  (Bit 1 set also routes f32 complex
 * N = 8192 rows to fft_split2_kernel: a development A/B switch.) */
PDSP_API int pdsp_set_split16k(int enabled);
/* Same kind of switch for 32 <= N <= 256 transforms on 16-byte aligned planes: 1 (default) =
 * fft_staged_kernel (the workgroup's contiguous 4096-point chunk staged through LDS with coalesced
 * 16-byte accesses), 0 = the direct kernel. */
PDSP_API int pdsp_set_staged_small(int enabled);
/* 1 (default): a window argument that IS one of the plan's own tables (pdsp_plan_window_f32) is
 * evaluated inside the N = 16384 f32 spectrum kernel (createWindow fused, see below); 0: it is read
 * as a table like any caller-supplied window.  A/B switch for the parity tests; returns the
 * previous value. */
PDSP_API int pdsp_set_fused_window(int enabled);
/* 1 (default): f32 transforms of 2^15 <= N <= 2^27 on 16-byte aligned planes run as tile passes over
 * balanced factors of 64 ... 512 points (tile_pass_kernel): TWO passes over HBM up to 2^18, THREE above;
 * 0: round 1's four-step forms (N1 <= 16 columns, 16384-point rows, transposing copy: three passes up to
 * 2^18, five above); 3: tile passes in their first form -- the scratch planes between the first two of three
 * passes in natural order instead of tile-major (bit-identical results), 512-point factors on 16-wide tiles
 * instead of the 32-wide ones of tile_rows512_kernel / tile_cols512_kernel (same results within rounding).
 * With the value 1 only, 2^15 and 2^16 out of place run in ONE pass over HBM on fft_paired_kernel (2 / 4 sibling
 * workgroups per transform sharing an XCD's L2); 5 = the tile passes' current form without it.
 * A/B switch, returns the previous value. */
PDSP_API int pdsp_set_twopass(int enabled);

/* 1 (default): f64 Radix2Fft.forward rows (real input, src/core/fft.ts:77-79) of N = 8192, and of N = 16384 from 8
 * rows up (the device forms; the host forms: at every row count, so that a row's bits never depend on its batch),
 * run as ONE N/2-point packed-real transform per row + the split to X[k], X[k + N/2] (fft_real_kernel);
 * 0: as the complex kernel of their size on (x, 0) (fft_stockham_kernel with LoadReal; N = 16384: the four-step
 * path).  Same results within rounding.  Other sizes and f32 real rows always take the complex kernels
 * (DESIGN 4.1c). */
PDSP_API int pdsp_set_real_packed(int enabled);

/* Frames per chunk of the two-pass inverse short-time transform (pdsp_istft_*, hop < N): 0 (default) = the bound
 * stated in pdsp_hip.h, n >= 1 = n frames (capped so that a chunk's outputs fit one grid).  Results are bit-identical
 * for every value; tests use small ones to run many chunks on small inputs.  Returns the previous value. */
PDSP_API int pdsp_set_istft_chunk_frames(int frames);

/* The tile of the polyphase rate change (pdsp_upfirdn_*), forced.  mode & 15 is the instantiation:
 * 0 (default) = the tile rule, 1 = R = 4, 2 = R = 8 with the sliding window (WIN), 3 = R = 1, 4 = R = 1 with the taps
 * read from global memory (GT).  mode >> 4 caps B, the outputs per phase and tile: 0 = no cap, n = at most n rounded
 * up to a multiple of R (applied after the rule's own cap by the row's outputs; with instantiation 0 the rule then
 * chooses among the capped tiles).  A forced instantiation is never replaced: where it is not legal for a call (WIN
 * with down != 1) or has no tile within 160 KiB of LDS, the call fails with PDSP_ERR_UNSUPPORTED_SIZE before any
 * launch.  Results are bit-identical for every value; tests use it to run each instantiation, and many small tiles,
 * on small inputs.  A mode that is negative or names no instantiation leaves the setting as it is.  Returns the
 * previous value. */
PDSP_API int pdsp_set_upfirdn_tile(int mode);
/* The tile a pdsp_upfirdn_* call with these arguments (elem_bytes 4 or 8) would launch under the current
 * pdsp_set_upfirdn_tile: info = r, win, gt, tn, tp, bper, span, lds_bytes, items.  Needs no device.
 * 1 <= up, down, ntaps <= 8192, y_len >= 1. */
PDSP_API int pdsp_dev_upfirdn_tile(long long up, long long down, long long ntaps, long long y_len, int elem_bytes,
                                   long long info[9]);

/* The path and tile of the wavelet transform (pdsp_dwt_*), forced.  mode & 3: 0 (default) = the rule,
 * 1 = the resident path (rows up to 160 KiB of LDS), 2 = the tiled path.  mode >> 2 caps T, the positions per tile:
 * 0 = no cap, n = at most n rounded up to a multiple of 2^levels.  A forced path is never replaced: where it does not
 * fit (a row beyond LDS, a depth beyond the tiled path's limit) the call fails with PDSP_ERR_UNSUPPORTED_SIZE before
 * any launch.  Results are bit-identical for every value; tests use it to run both paths, and many small tiles whose
 * halo wraps round the row, on small inputs.  A mode that is negative or names no path leaves the setting as it is.
 * Returns the previous value. */
PDSP_API int pdsp_set_dwt_tile(int mode);
/* What a pdsp_dwt_forward_* (inverse = 0) or pdsp_dwt_inverse_* (inverse = 1) call would launch under the current
 * pdsp_set_dwt_tile: info = resident (1 / 0), T, halo (forward: samples staged beyond T; inverse: coefficients in front
 * of a tile per band), lds_bytes, tiles per row.  Needs no device.  len a positive multiple of 2^levels. */
PDSP_API int pdsp_dev_dwt_tile(long long ntaps, int levels, long long len, int elem_bytes, int inverse,
                               long long info[5]);

/* Which complex_op_kernel instantiation a pdsp_complex_op_f32 call with these arguments launches: *vec4 = 1 for
 * four values per thread in 16-byte accesses (a_re, a_im, out_re, out_im, and for a binary op b_re, b_im, all on
 * 16-byte boundaries; count, and for a binary op b_len, multiples of 4), 0 for one value per thread.  The pointers
 * are only looked at.  Needs no device. */
PDSP_API int pdsp_dev_complex_op_vec4(int op, long long count, const float *a_re, const float *a_im,
                                      const float *b_re, const float *b_im, long long b_len, const float *out_re,
                                      const float *out_im, int *vec4);

/* What a pdsp_fft_forward_real_* / _forward_complex_* / _inverse_* call (pdsp_dev_transform_path_*: the planes in that
 * entry point's order, im_in null for real rows, inverse = 1 for pdsp_fft_inverse_*) or a pdsp_spectrum_* /
 * pdsp_spectrum_peaks_f32 call (pdsp_dev_spectrum_path_*: peak_idx_out and peaks_out as the call has them, the other
 * null) would run on these very pointers under the current switches.  The queries run the call's own argument checks
 * -- a call that is refused is refused here with the same code and text -- and then the decision function the call
 * itself switches on (pdsp_dispatch.inc: Pick), and write it to info.  They launch nothing and
 * allocate nothing; the pointers are only looked at.  An empty batch gives path 0.  info, PDSP_DEV_PATH_INFO ints:
 *   [0] path: 1 fft_tiny_staged_kernel, 2 fft_staged_kernel, 3 fft_stockham_kernel, 4 fft_split2_kernel,
 *       5 fft_split4_kernel, 6 fft_real_kernel (f64 packed-real rows), 7 fft_paired_kernel, 8 two or three tile passes,
 *       9 fused four-step (fourstep_cols_kernel, N2-point rows, fourstep_out_kernel), 10 general four-step
 *       (bigfft_transpose_kernel around N1- and N2-point rows); spectra: 9 and 10 with amplitude rows from the last
 *       pass, 11 memset (empty frames), 12 packed-real frames on tile passes + split_amp_rows_kernel,
 *       13 spectrum_staged_kernel, 14 spectrum_dif16k_kernel, 15 spectrum_packed_kernel, 16 fft_tiny_staged_kernel
 *       with amplitude store, 17 the complex kernel on (x, 0) with amplitude store (N < 64)
 *   [1] rows: the rows kernel as a path value 3 ... 5 -- paths 3 ... 5: the path itself; 9 and 10: of the N2-point rows
 *   [2] n1_rows: path 10, the kernel of the N1-point rows, 2 ... 5; [3] n1_square: 1 = N1 == N2, they run like the
 *       N2-point rows on the same tables, 0 = on the N1-point tables of their own
 *   [4] np: tile passes run (path 8; path 12 with head 0); [5..7] tile: each pass's kernel, 1 tile_pass_kernel,
 *       2 tile_cols512_kernel, 3 tile_rows512_kernel; [8] tile_major: the planes between the first two of three passes
 *       are tile-major, not in natural order
 *   [9] pairs: scratch plane pairs drawn; [10] out_first: the output planes serve as the first intermediate pair
 *       (paths 8 with three passes and 10, transforms only: output and input share no bytes)
 *   [11] fast: paths 13 ... 15, whole pair-aligned one-sided frames without phase rows; [12] wmode: the same paths,
 *       0 rect, 1 window table, 2 / 3 fused two- / three-term cosine sum
 *   [13] first: path 12, the first pass's loader, 3 rect, 4 window table, 5 / 6 fused two- / three-term cosine sum
 *   [14] fused_peaks: paths 14 and 15, the peak records are written by the spectrum kernel itself
 *   [15] peaks: the kernels that run on the stored rows afterwards, bits 1 peak_wave_kernel, 2 find_peak_kernel,
 *       4 peak_from_rows_kernel
 *   [16] head: path 12, what runs the N/2-point transform: 0 the tile passes of [4..8], 1 fft_split4_kernel with the
 *       packed loader, 2 fft_paired_kernel with the packed loader */
#define PDSP_DEV_PATH_INFO 17
PDSP_API int pdsp_dev_transform_path_f32(const pdsp_plan *plan, long long batch, const float *re_in, const float *im_in,
                                         const float *re_out, const float *im_out, int inverse,
                                         int info[PDSP_DEV_PATH_INFO]);
PDSP_API int pdsp_dev_transform_path_f64(const pdsp_plan *plan, long long batch, const double *re_in,
                                         const double *im_in, const double *re_out, const double *im_out, int inverse,
                                         int info[PDSP_DEV_PATH_INFO]);
PDSP_API int pdsp_dev_spectrum_path_f32(const pdsp_plan *plan, long long batch, const float *frames, long long frame_len,
                                        long long frame_stride, const float *window, int sides, const float *amp_out,
                                        const float *phase_out, const int32_t *peak_idx_out,
                                        const pdsp_peak32 *peaks_out, double sample_rate, int info[PDSP_DEV_PATH_INFO]);
PDSP_API int pdsp_dev_spectrum_path_f64(const pdsp_plan *plan, long long batch, const double *frames,
                                        long long frame_len, long long frame_stride, const double *window, int sides,
                                        const double *amp_out, const double *phase_out, const int32_t *peak_idx_out,
                                        const pdsp_peak32 *peaks_out, double sample_rate, int info[PDSP_DEV_PATH_INFO]);

/* How a batched host call would be cut under the current PDSP_HOST_THREADS (read at the call, like the calls do):
 * pdsp_fft_transform_host_f64 / _rows_host_f64 of `batch` rows on this plan, or pdsp_spectrum_batch_host_f64 /
 * _rows_host_f64 / _rows_host_f32in of `batch` non-empty frames at this plan's size, in host precision 32 or 64 (a size
 * beyond the f64 tables runs in f32, as in the calls).  info[0] = rows per chunk -- the last chunk holds the
 * remainder -- and info[1] = workers; both 0 when the call keeps the one-shot sequence (as it also does, whatever this
 * says, when its planes overlap in host memory).  The calls ask the same function.  Launches nothing; needs no
 * device beyond the plan's. */
PDSP_API int pdsp_dev_host_transform_chunks(const pdsp_plan *plan, long long batch, int precision, long long info[2]);
PDSP_API int pdsp_dev_host_spectrum_chunks(const pdsp_plan *plan, long long batch, int sides, int precision,
                                           long long info[2]);

/* What the library holds at this moment, counted exactly (std::atomic counters touched where a resource is created or
 * freed and nowhere on a launch path): the tests of re-entrancy, of the plan cache and of handle lifetimes compare
 * them before and after.  info, PDSP_DEV_LIVE_INFO values:
 *   [0] plans in the host forms' cache (at most 16 unless every entry is in use); [1] of those, entries a call is
 *       running on right now (pinned: never evicted, kept by pdsp_plan_cache_clear)
 *   [2] cached plans evicted to make room for another size since the library was loaded (pdsp_plan_cache_clear's
 *       frees are not evictions)
 *   [3] device tables alive -- every allocation a plan, a resampler, a dft, a czt, a dwt, an ntt or an sdft handle
 *       uploaded and has not yet freed -- and [4] their bytes
 *   [5] pinned host staging buffers and [6] device staging buffers of plans (the host-f64 transform and spectrum forms)
 *   [7] streams the library created (a plan's own, and its slot streams of chunked host calls)
 * The cache entries are read under the cache's lock; the rest are single atomic loads, so with calls in flight the
 * values are each exact but not one snapshot.  Launches nothing, allocates nothing, needs no device. */
#define PDSP_DEV_LIVE_INFO 8
PDSP_API int pdsp_dev_live_resources(long long info[PDSP_DEV_LIVE_INFO]);

#ifdef __cplusplus
}
#endif
#endif /* PDSP_HIP_DEV_H */

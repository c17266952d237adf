/*
 * pdsp_hip.h -- C ABI of the MI355X (gfx950) batched FFT / spectrum engine that
 * re-backs pragma-dsp's hot path.  Plain pointers and sizes only; no torch, no
 * C++ types.  Built as pragma-dsp_amd/csrc/libpdsp_hip.so.
 *
 * Every entry point cites the reference interface (relative to the pragma-dsp
 * repository) whose work it replaces.  The reference has no FFI today (it is
 * pure TypeScript); the binding a maintainer would add (N-API addon) is in
 * pragma-dsp_amd/csrc/pdsp_napi.c and is described in INTEGRATION.md.
 *
 * Conventions (src/core/fft.ts:89-151, PLAN.md:104-128):
 *   forward  X[k] = sum_n x[n] e^{-j 2 pi k n / N}   (no normalisation)
 *   inverse  x[n] = (1/N) sum_k X[k] e^{+j 2 pi k n / N}
 *   complex data is PLANAR {real[], imag[]} like the reference's ComplexArray;
 *   a batch is `batch` rows of N contiguous values: re[b*N + i], im[b*N + i].
 *
 * Two families:
 *   *_f32 / *_f64 with `pdsp_stream`  -- DEVICE pointers, asynchronous on the
 *       given HIP stream (0 = the null stream).  This is the throughput path
 *       (bench, batched callers).
 *   *_host_f64                        -- HOST f64 pointers, synchronous.  This
 *       is what the JS drop-in (`Radix2Fft`, `FFT`, `spectrum`) binds: the
 *       reference API is Float64Array in / Float64Array out.
 *
 * Return value: 0 (PDSP_OK) or a pdsp_status; pdsp_last_error() then returns a
 * thread-local message.  For the argument errors the reference throws on, the
 * message is the reference's exact text, and validation happens before any
 * device work.
 */
#ifndef PDSP_HIP_H
#define PDSP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDSP_API __attribute__((visibility("default")))

typedef struct pdsp_plan pdsp_plan; /* replaces a Radix2Fft instance, src/core/fft.ts:63-75 */
typedef void *pdsp_stream;          /* a hipStream_t, passed as an opaque pointer */

typedef enum pdsp_status {
  PDSP_OK = 0,
  PDSP_ERR_SIZE_NOT_POW2 = 1,   /* "FFT size must be power of two, got ${size}"  fft.ts:69-71, fourier.ts:74-76 */
  PDSP_ERR_INPUT_LENGTH = 2,    /* "FFT input length ${len} != size ${N}"         fft.ts:95-104 */
  PDSP_ERR_WINDOW_SIZE = 3,     /* "Window size must be positive, got ${size}"    fourier.ts:15-17 */
  PDSP_ERR_WINDOW_LENGTH = 4,   /* "Window length must match input length."       fourier.ts:59-61 */
  PDSP_ERR_WINDOW_TYPE = 5,     /* "Unsupported window type: ${t}"                fourier.ts:47-50 */
  PDSP_ERR_FFT_SIZE = 6,        /* "FFT size must be positive, got ${size}"       fourier.ts:152-154 */
  PDSP_ERR_SAMPLE_RATE = 7,     /* "Sample rate must be positive, got ${sr}"      fourier.ts:155-157 */
  PDSP_ERR_UNSUPPORTED_SIZE = 8,/* power of two, but beyond pdsp_max_size() for that precision */
  PDSP_ERR_BAD_ARG = 9,         /* null pointer / negative batch */
  PDSP_ERR_DEVICE = 10          /* no GPU, or a HIP runtime error (message has the HIP text) */
} pdsp_status;

typedef enum pdsp_window {      /* WindowType, src/xform/fourier.ts:11 */
  PDSP_WIN_RECT = 0,
  PDSP_WIN_HANN = 1,
  PDSP_WIN_HAMMING = 2,
  PDSP_WIN_BLACKMAN = 3
} pdsp_window;

typedef enum pdsp_sides {       /* FftSides, src/xform/fourier.ts:12 */
  PDSP_SIDES_ONE = 0,
  PDSP_SIDES_TWO = 1
} pdsp_sides;

typedef struct pdsp_peak {      /* SpectrumPeak, src/public/spectrum.ts:15-20 */
  int32_t index;
  double frequency;
  double amplitude;
  double phase;
} pdsp_peak;

typedef struct pdsp_peak32 {    /* SpectrumPeak of one frame as the device writes it (16 bytes) */
  int32_t index;
  float frequency;
  float amplitude;
  float phase;
} pdsp_peak32;

/* ---- library ---------------------------------------------------------- */

PDSP_API int pdsp_version(void);
PDSP_API const char *pdsp_last_error(void);
/* Number of visible HIP devices (0 when there is none); never fails. */
PDSP_API int pdsp_device_count(void);
/* Largest N for 4-byte / 8-byte scalars: 2^28 / 2^26.  Up to 16384 / 8192 (16384 for the f64
 * real-frame spectrum) one LDS-resident pass; up to 16x that a three-pass four-step transform
 * (columns fused into one kernel); above, the general five-pass four-step (both factors on the
 * row kernels, tiled transposes between them). */
PDSP_API int pdsp_max_size(int scalar_bytes);

/* Arithmetic of the *_host_f64 entry points (process-wide; returns the previous value).
 *   64 (default): f64 on the device for every size up to 2^26 -- the drop-in then meets the
 *       reference's own test tolerances (1e-10 against NumPy, signals.test.ts:22-23), not just the
 *       f32 contract; N = 2^27, 2^28 compute in f32.
 *   32: always f32 (the north-star's stated contract, max|err|/max|X| <= 1e-5).
 * PDSP_HOST_PRECISION=32 in the environment presets it. */
PDSP_API int pdsp_set_host_precision(int bits);

/* ---- host-side index math (no device) --------------------------------- */

/* isPowerOfTwo, src/core/fft.ts:16 (integers only). */
PDSP_API int pdsp_is_pow2(long long n);
/* nextPowerOfTwo, src/core/fft.ts:18-23 (no int32 overflow). */
PDSP_API long long pdsp_next_pow2(long long n);
/* createWindow, src/xform/fourier.ts:14-52.  Host, f64 (an f32 window misses
 * the reference's 1e-8 window tolerance). */
PDSP_API int pdsp_window_make(int type, long long size, double *out);
/* binFrequencies, src/xform/fourier.ts:147-165.  `out` holds size/2+1 (one) or
 * size (two) values; *bins_out receives the count. */
PDSP_API int pdsp_bin_frequencies(long long size, double sample_rate, int sides,
                                  double *out, long long *bins_out);
/* fftShift, src/xform/fourier.ts:122-134: out[i] = in[(i + floor(n/2)) % n]. */
PDSP_API int pdsp_fft_shift_f64(const double *in, long long n, double *out);
/* findPeak, src/public/spectrum.ts:74-105 (strict '>', DC skipped unless no
 * other bin is > 0).  Returns the index (>= 0). */
PDSP_API long long pdsp_find_peak_f64(const double *amplitude, long long bins);

/* ---- plan -------------------------------------------------------------- */

/* new Radix2Fft(size) / new FFT(size): src/core/fft.ts:68-75,
 * src/xform/fourier.ts:73-79.  Builds the twiddle tables on the host in f64 and
 * uploads them to `device` (-1 = the current HIP device).  The bit-reversal
 * table of fft.ts:25-38 has no counterpart: the Stockham kernel autosorts. */
PDSP_API int pdsp_plan_create(long long size, int device, pdsp_plan **plan_out);
PDSP_API int pdsp_plan_destroy(pdsp_plan *plan);
PDSP_API long long pdsp_plan_size(const pdsp_plan *plan);
/* pdsp_spectrum_host_f64 keeps its plans and device windows in a process-wide cache keyed
 * by (size, device) -- the FourierLive idea, src/effect/index.ts:30-48 (the reference's
 * spectrum() rebuilds plan and window on every call, spectrum.ts:114-116).  This frees it, and hands the
 * scratch planes the multi-pass paths (N > 16384) keep in the engine's own stream-ordered memory pool -- as large
 * as the largest such transform run so far -- back to the device. */
PDSP_API int pdsp_plan_cache_clear(void);
PDSP_API int pdsp_plan_device(const pdsp_plan *plan);

/* The plan's own device copy of createWindow(type, N) (src/xform/fourier.ts:14-52; built in f64 on
 * the host, rounded once, uploaded on first use, owned by the plan and valid for its lifetime) -- the
 * Map<"type:size", window> of FourierLive (src/effect/index.ts:39-48) per plan.  Passing this pointer
 * as `window` to pdsp_spectrum_f32 / pdsp_spectrum_peaks_f32 tells the engine WHICH window it is: for
 * N = 16384 f32 frames the cosine-sum window a0 - a1 cos(2 pi n/(N-1)) + a2 cos(4 pi n/(N-1)) is then
 * evaluated in registers (createWindow + applyWindow fused into the frame load; values agree with
 * the table to ~2e-7 absolute) instead of being re-read, 64 KB per frame, from L2.  Any other
 * pointer is used as a table of N values.
 * The first call for a type uploads the table with a synchronous allocation and copy, and the call takes no stream: a
 * caller who captures a stream into a graph fetches the plan's windows before beginning the capture. */
PDSP_API int pdsp_plan_window_f32(pdsp_plan *plan, int type, const float **window_out);
PDSP_API int pdsp_plan_window_f64(pdsp_plan *plan, int type, const double **window_out);

/* ---- plane layout ------------------------------------------------------- */

/* Device memory for the four planes of a batched transform, laid out for this card's memory system: inside one large
 * allocation the MI355X address space behaves as regions of 32 GiB, and a transform that streams two input planes
 * and two output planes runs fastest -- 79-83 % of the HBM roofline at N = 4096, repeatable, against 71-84 % by
 * lottery for four separate allocations -- with both INPUT planes in one region and each OUTPUT plane in a region
 * of its own.  One allocation of 80 GiB + a plane: re_in at 0, im_in right behind it, re_out
 * 40 GiB in, im_out 80 GiB in (any phase of the allocation against the region grid then puts the outputs one and two
 * regions beyond the inputs).  When that much memory is not free, or a plane is below 256 MiB (nothing to gain) or
 * above 8 GiB: four plain allocations.
 *   scalar_bytes  4 (float planes) or 8 (double planes); each plane holds batch * N scalars
 *   real_input    non-zero: no imaginary input plane (*im_in = NULL)
 *   *arena        opaque handle for pdsp_planes_free (which frees all four planes); *arena_bytes (may be NULL)
 *                 receives the size of the one allocation, 0 for the plain-allocation fallback
 * Nothing in the reference corresponds to this: it is a property of the device, not of the algorithm. */
typedef struct pdsp_arena pdsp_arena;
PDSP_API int pdsp_planes_alloc(const pdsp_plan *plan, long long batch, int scalar_bytes, int real_input,
                               void **re_in, void **im_in, void **re_out, void **im_out,
                               pdsp_arena **arena, unsigned long long *arena_bytes);
PDSP_API int pdsp_planes_free(pdsp_arena *arena);

/* ---- device-pointer batched transforms (f32) --------------------------- */

/* Aliasing, for every transform of this section and its f64 twin (DESIGN.md 4.1d has the reasoning
 * kernel by kernel).  Planes are compared as byte ranges of batch * N scalars.
 *   Single-pass sizes (N <= 16384 in f32, N <= 8192 in f64, and f64 real rows of N = 16384 at every
 *   batch): an output plane may share bytes with an input plane only where the two begin at the same
 *   address.  That admits the exact in-place call (re_out == re_in, im_out == im_in), the exchanged
 *   one (re_out == im_in, im_out == re_in), either output plane alone on either input plane, and for
 *   real rows re_out == re_in or im_out == re_in.  Each workgroup loads its rows whole before it
 *   stores them, but no workgroup waits for another: an output that starts one element, one row or
 *   half a plane into an input would race, and is refused.
 *   Larger sizes run in several passes through planes of their own: any overlap of an output with an
 *   input is accepted and correct.
 *   At every size re_out and im_out must not overlap each other.
 *   Interleaved rows: out == in is the one overlap allowed.
 * Anything else is refused with PDSP_ERR_BAD_ARG before anything is launched -- "output overlaps
 * input (an output plane may share bytes with an input plane only where the two begin at the same
 * address)", "output overlaps input (only out == in may share bytes)" or "the output planes overlap
 * each other" -- and pdsp_dev_transform_path_* (pdsp_hip_dev.h) refuses the same calls with the same
 * text.  Buffers that touch without overlapping are legal. */

/* Radix2Fft.forward(input) row by row, src/core/fft.ts:77-79: real input,
 * imaginary part taken as zero.  re_in[batch*N] -> re_out, im_out[batch*N]. */
PDSP_API int pdsp_fft_forward_real_f32(const pdsp_plan *plan, long long batch,
                                       const float *re_in, float *re_out, float *im_out,
                                       pdsp_stream stream);
/* Radix2Fft.forwardComplex, src/core/fft.ts:81-83.
 * Where the four planes lie matters on this card (8-14 % at N = 4096): inside one large allocation the address space
 * behaves as regions of 32 GiB, and the launch is fastest -- and repeatable -- with both input planes in one region
 * and each output plane in a region of its own, e.g. offsets 0 / plane / 40 GiB / 80 GiB of one allocation
 * (pragma_dsp_amd.batch.BatchedFft.alloc_planes does exactly that). */
PDSP_API int pdsp_fft_forward_complex_f32(const pdsp_plan *plan, long long batch,
                                          const float *re_in, const float *im_in,
                                          float *re_out, float *im_out, pdsp_stream stream);
/* The same forwardComplex / inverse on INTERLEAVED rows: in/out hold batch*N (re, im) pairs
 * (2*N scalars per row) -- the layout of I/Q streams and complex64 tensors.  An extension: the
 * reference's ComplexArray is planar (src/core/fft.ts:1-4).  Single-pass sizes only (N <= 16384
 * in f32, 8192 in f64; PDSP_ERR_UNSUPPORTED_SIZE beyond); out == in runs in place, any other overlap
 * of out with in is refused (see "Aliasing" above). */
PDSP_API int pdsp_fft_forward_interleaved_f32(const pdsp_plan *plan, long long batch, const float *in,
                                              float *out, pdsp_stream stream);
PDSP_API int pdsp_fft_inverse_interleaved_f32(const pdsp_plan *plan, long long batch, const float *in,
                                              float *out, pdsp_stream stream);
/* Radix2Fft.inverse (conjugate twiddles + 1/N), src/core/fft.ts:85-87, :142-148. */
PDSP_API int pdsp_fft_inverse_f32(const pdsp_plan *plan, long long batch,
                                  const float *re_in, const float *im_in,
                                  float *re_out, float *im_out, pdsp_stream stream);

/* ---- device-pointer elementwise helpers (f32) -------------------------- */

/* Aliasing, for every helper of this section and its f64 twin: an output may share bytes with an
 * input of the same extent only where the two begin at the same address (each element is read
 * before it is written); any other overlap is refused with PDSP_ERR_BAD_ARG, "output overlaps
 * input", before anything is launched. */

/* applyWindow row by row, src/xform/fourier.ts:54-67: out[b][i] = in[b][i]*win[i].  out == in is
 * allowed; out partially overlapping in, or overlapping window, is refused, and so is a batch * n
 * that overflows. */
PDSP_API int pdsp_apply_window_f32(long long batch, long long n, const float *in,
                                   const float *window, float *out, pdsp_stream stream);
/* magnitude, src/xform/fourier.ts:98-109 (sqrt(re^2+im^2), the sum of squares rounded
 * to f32 once and its f32 sqrt; not the overflow-safe hypot, and a NaN operand gives NaN
 * whatever the other is).  Within 1 ulp while re^2 + im^2 is a normal f32:
 * 1.1e-19 <= |X| <= 1.8e19.  The fused amplitude stores of pdsp_spectrum_f32 /
 * pdsp_spectrum_peaks_f32 square either the bin or half its scaled amplitude, so
 * their rows hold for |X_k| <= 1.8e19 and amplitudes >= 2.2e-19; see DESIGN.md §1. */
PDSP_API int pdsp_magnitude_f32(long long count, const float *re, const float *im,
                                float *out, pdsp_stream stream);
/* phase, src/xform/fourier.ts:111-120: atan2(im, re).  For magnitude and phase alike, out == re
 * or out == im is allowed; out partially overlapping either is refused. */
PDSP_API int pdsp_phase_f32(long long count, const float *re, const float *im,
                            float *out, pdsp_stream stream);

/* Element-wise complex vector arithmetic on planar device rows, src/math/complex.ts:26-197
 * (scaleInto, addInto, subInto, mulInto, mulScalarInto, divInto, conjInto), so FFT-domain
 * pipelines (forward -> mul -> inverse, test/fluent/chain.test.ts:287-317) stay in HBM.
 * out = a OP b for the binary ops, where b holds b_len values and is broadcast over the
 * count/b_len rows of a when b_len < count (b_len must divide count); out = a OP (s_re, s_im)
 * for SCALE (real s_re) and MUL_SCALAR; out = conj(a) for CONJ.  divScalar is MUL_SCALAR by the
 * host-computed reciprocal, as complex.ts:176-186 does.  out may alias a, and b may alias out when
 * b_len == count (every element is read before it is written); a broadcast b (b_len < count) must
 * not overlap out.  Enforced plane by plane: an out plane may share bytes with a_re, a_im, or with
 * b_re / b_im when b_len == count, only where the two planes begin at the same address (exact in
 * place, a == b == out, and out_re == a_im with out_im == a_re are all allowed); out_re and out_im
 * must not overlap each other; a broadcast b must share no byte with either out plane.  Anything
 * else is refused with PDSP_ERR_BAD_ARG, "output overlaps input".  b is ignored by the unary ops. */
typedef enum pdsp_complex_op {
  PDSP_CX_ADD = 0, PDSP_CX_SUB = 1, PDSP_CX_MUL = 2, PDSP_CX_DIV = 3,
  PDSP_CX_CONJ = 4, PDSP_CX_SCALE = 5, PDSP_CX_MUL_SCALAR = 6
} pdsp_complex_op;
PDSP_API int pdsp_complex_op_f32(int op, long long count, const float *a_re, const float *a_im,
                                 const float *b_re, const float *b_im, long long b_len,
                                 double s_re, double s_im, float *out_re, float *out_im,
                                 pdsp_stream stream);

/* ---- fused spectrum (f32) ---------------------------------------------- */

/* The batched body of spectrum(), src/public/spectrum.ts:116-131, one frame per
 * row, fused in one kernel: buildFrame (zero-pad / truncate to N, :36-43) ->
 * applyWindow -> forward FFT -> magnitude -> one-/two-sided amplitude scaling
 * (:45-72) [-> phase, :122,128-131] [-> findPeak index, :74-105].
 *   frames      [batch][frame_stride] real samples; the first
 *               min(frame_len, N) of each row are used, the rest is zero.
 *               frame_stride >= 1: a stride below frame_len reads OVERLAPPING frames of one
 *               signal (a short-time transform with hop = frame_stride; frame b starts at
 *               sample b*frame_stride and the buffer must hold (batch-1)*frame_stride +
 *               min(frame_len, N) samples).
 *   window      N device floats, or NULL for "rect".
 *   amp_out     [batch][bins], bins = N/2+1 (one-sided) or N (two-sided).
 *   phase_out   same shape, or NULL.
 *   peak_out    [batch] int32 peak bin per frame, or NULL.
 * Aliasing (pdsp_spectrum_f32 / _f64 and pdsp_spectrum_peaks_f32, at every size): there is no
 * in-place form.  amp_out, phase_out and peak_out / peaks_out share no byte with the frames' extent
 * -- (batch-1)*frame_stride + min(frame_len, N) samples --, with the window's N values or with each
 * other; a call that does is refused with PDSP_ERR_BAD_ARG, "output overlaps input (the spectrum has
 * no in-place form)" or "the outputs overlap each other", before anything is launched, and by
 * pdsp_dev_spectrum_path_* alike.  An output that begins right behind the last sample is legal. */
PDSP_API int pdsp_spectrum_f32(const pdsp_plan *plan, long long batch,
                               const float *frames, long long frame_len, long long frame_stride,
                               const float *window, int sides,
                               float *amp_out, float *phase_out, int32_t *peak_out,
                               pdsp_stream stream);

/* The whole tail of spectrum() on the device (src/public/spectrum.ts:116-134), one
 * SpectrumPeak per frame: findPeak (:74-105: bins >= 1, strict '>', the first of equal
 * values wins, bin 0 when no other bin is > 0) is fused into the spectrum kernel, with
 * peak.frequency = index * sample_rate / N and peak.phase = atan2 of that bin.
 *   peaks_out   [batch] records (16 B each).
 *   amp_out / phase_out   optional [batch][bins] rows as in pdsp_spectrum_f32; NULL for
 *               peaks-only output: HBM traffic is then 4 B/sample in + 16 B/frame out, and a
 *               multi-GPU gather moves KiBs instead of GiBs.
 * In two-sided mode bins k and N-k carry identical values here, so the peak is the lower
 * index k (the reference picks whichever f64 rounding favours). */
PDSP_API int pdsp_spectrum_peaks_f32(const pdsp_plan *plan, long long batch,
                                     const float *frames, long long frame_len, long long frame_stride,
                                     const float *window, int sides, double sample_rate,
                                     float *amp_out, float *phase_out, pdsp_peak32 *peaks_out,
                                     pdsp_stream stream);

/* ---- the same device-pointer family in f64 ------------------------------ */
/* Identical contracts with double rows, N <= 2^26 (PDSP_ERR_UNSUPPORTED_SIZE beyond).
 * Per bin, 2.3e-16 * log2 N of the row's rms at most (measured against long-double references).
 * pdsp_fft_forward_real_f64 at N = 16384 runs one kernel variant from 8 rows up and another below, so there the variant,
 * and with it the last bits of a row, depend on the batch (pdsp_dev_transform_path_f64 in pdsp_hip_dev.h names it); the
 * host entry points below choose by size alone, and a row's bits never depend on its batch. */
PDSP_API int pdsp_fft_forward_real_f64(const pdsp_plan *plan, long long batch,
                                       const double *re_in, double *re_out, double *im_out,
                                       pdsp_stream stream);
PDSP_API int pdsp_fft_forward_complex_f64(const pdsp_plan *plan, long long batch,
                                          const double *re_in, const double *im_in,
                                          double *re_out, double *im_out, pdsp_stream stream);
PDSP_API int pdsp_fft_inverse_f64(const pdsp_plan *plan, long long batch,
                                  const double *re_in, const double *im_in,
                                  double *re_out, double *im_out, pdsp_stream stream);
PDSP_API int pdsp_fft_forward_interleaved_f64(const pdsp_plan *plan, long long batch, const double *in,
                                              double *out, pdsp_stream stream);
PDSP_API int pdsp_fft_inverse_interleaved_f64(const pdsp_plan *plan, long long batch, const double *in,
                                              double *out, pdsp_stream stream);
PDSP_API int pdsp_apply_window_f64(long long batch, long long n, const double *in,
                                   const double *window, double *out, pdsp_stream stream);
/* f64 magnitude is hypot(re, im) like the reference's Math.hypot (fourier.ts:106): no overflow /
 * underflow of the squares at the ends of the double range. */
PDSP_API int pdsp_magnitude_f64(long long count, const double *re, const double *im,
                                double *out, pdsp_stream stream);
PDSP_API int pdsp_phase_f64(long long count, const double *re, const double *im,
                            double *out, pdsp_stream stream);
PDSP_API int pdsp_spectrum_f64(const pdsp_plan *plan, long long batch,
                               const double *frames, long long frame_len, long long frame_stride,
                               const double *window, int sides,
                               double *amp_out, double *phase_out, int32_t *peak_out,
                               pdsp_stream stream);

/* ---- host f64 drop-in entry points (synchronous) ----------------------- */

/* Radix2Fft.transform, src/core/fft.ts:89-151, for `batch` rows.  im_in may be
 * NULL (= forward(real)).  in_len is the caller's row length and must equal N
 * (PDSP_ERR_INPUT_LENGTH otherwise, message as fft.ts:95-104).  Computes on the
 * device in the precision pdsp_set_host_precision() selects (f64 at the boundary either way).
 * Row b equals the one-row call on row b bit for bit, at every batch and however the call is cut into chunks. */
PDSP_API int pdsp_fft_transform_host_f64(pdsp_plan *plan, long long batch, long long in_len,
                                         const double *re_in, const double *im_in,
                                         double *re_out, double *im_out, int inverse);
/* The same with one pointer per input row (re_rows[b], and im_rows[b] unless im_rows is NULL, point at N values
 * each, anywhere in host memory): a JS array of Float64Arrays / ComplexArrays taken where it lies.  Outputs are
 * contiguous planes of batch*N values as above. */
PDSP_API int pdsp_fft_transform_rows_host_f64(pdsp_plan *plan, long long batch, long long in_len,
                                              const double *const *re_rows, const double *const *im_rows,
                                              double *re_out, double *im_out, int inverse);
/* applyWindow / magnitude / phase on host arrays (fourier.ts:54-67, :98-120).
 * Small inputs: done by launching the same device kernels. */
PDSP_API int pdsp_apply_window_host_f64(const double *in, long long in_len, const double *window,
                                        long long window_len, double *out);
PDSP_API int pdsp_magnitude_host_f64(const double *re, const double *im, long long n, double *out);
PDSP_API int pdsp_phase_host_f64(const double *re, const double *im, long long n, double *out);
/* spectrum(samples, options), src/public/spectrum.ts:107-142.  fft_size < 0
 * means "absent" = nextPowerOfTwo(len) (0 is rejected like `new FFT(0)`).  freq/amp/phase hold bins values (N/2+1 or N);
 * *bins_out receives the count.  Peak search runs on the host over the
 * f64-promoted amplitudes so the strict-'>' / first-wins rules are exact. */
PDSP_API int pdsp_spectrum_host_f64(const double *samples, long long len, double sample_rate,
                                    long long fft_size, int window, int sides,
                                    double *freq_out, double *amp_out, double *phase_out,
                                    pdsp_peak *peak_out, long long *bins_out);
/* The same on `batch` frames of `len` samples each (contiguous) in ONE call -- the map of the
 * reference's spectrumStream (src/effect/index.ts:190-194) batched onto the device.  freq_out holds
 * the one frequency axis (bins values); amp_out / phase_out batch*bins; peak_out batch records.
 * Row b equals pdsp_spectrum_host_f64 on frame b bit for bit.  Calls with 4 MiB or more of staging are cut into
 * chunks that several host threads (PDSP_HOST_THREADS; default half the cores, 2 ... 6; 1 = none) stage, copy and
 * launch concurrently on streams of their own -- the results do not depend on it. */
PDSP_API int pdsp_spectrum_batch_host_f64(const double *frames, long long batch, long long len,
                                          double sample_rate, long long fft_size, int window, int sides,
                                          double *freq_out, double *amp_out, double *phase_out,
                                          pdsp_peak *peak_out, long long *bins_out);

/* The same with ONE POINTER PER FRAME: rows[b] points at the `len` samples of frame b, anywhere in host memory --
 * the Iterable<ArrayLike<number>> of spectrumStream (src/effect/index.ts:190-194) as a JS caller holds it, an array
 * of Float64Arrays, taken as it stands instead of being flattened into one buffer first (a copy of 8 bytes per
 * sample on the caller's one thread).  Same outputs, same bit-for-bit rule. */
PDSP_API int pdsp_spectrum_rows_host_f64(const double *const *rows, long long batch, long long len,
                                         double sample_rate, long long fft_size, int window, int sides,
                                         double *freq_out, double *amp_out, double *phase_out,
                                         pdsp_peak *peak_out, long long *bins_out);

/* The same for frames held as 32-bit floats (Float32Array: what Web Audio, decoders and capture APIs hand a JS
 * caller; `ArrayLike<number>` in the reference's signature): rows[b] points at `len` floats.  The samples are widened
 * exactly (float -> double is exact) where the call computes in f64, and taken as they are in f32 mode, so the
 * results equal those of the f64 entry points on the widened frames bit for bit; outputs stay f64. */
PDSP_API int pdsp_spectrum_rows_host_f32in(const float *const *rows, long long batch, long long len,
                                           double sample_rate, long long fft_size, int window, int sides,
                                           double *freq_out, double *amp_out, double *phase_out,
                                           pdsp_peak *peak_out, long long *bins_out);

/* ---- FIR filtering (fused overlap-save), f32 / f64 ------------------------ */
/* Linear convolution y = x * h of many real rows with one real FIR filter of ntaps taps: the
 * "FIR helpers, convolution ... frequency response analysis via FFT utilities" of the reference's
 * roadmap (ROADMAP.md, "Filters and utilities": the pragma-dsp/filters module); the reference has
 * no such function yet.  Its FFT-domain form there is forward -> multiply -> inverse
 * (test/fluent/chain.test.ts:287-317); here that chain runs as ONE launch per call: each block of
 * N = pdsp_plan_size() samples is loaded once, transformed (packed-real, N/2 points), multiplied by
 * H, transformed back and its last N - ntaps + 1 samples stored -- overlap-save with
 * hop = N - ntaps + 1, nothing in between in HBM.  Filters longer than N/2 taps (partitioned
 * convolution) are not supported: PDSP_ERR_UNSUPPORTED_SIZE.  So are IIR filters, per-row filters,
 * complex signals and state carried across calls.
 * Validation happens before any device work: ntaps < 1, a negative batch / length / offset / stride,
 * outputs beyond the full convolution, a batch whose extent overflows 64 bits or whose blocks
 * overflow the grid give PDSP_ERR_BAD_ARG; a plan outside 64 <= N <= 16384 or ntaps > N/2 gives
 * PDSP_ERR_UNSUPPORTED_SIZE.  f32: ~1e-7 of max|x| * sum|h|; f64: ~1e-16. */

/* H[k] = sum_j taps[j] e^{-j 2 pi j k / N}, k = 0 ... N/2 (N/2 + 1 device values per plane): the
 * filter's frequency response sampled at the plan's N -- what pdsp_fir_filter_* reads, and useful on
 * its own.  Computed once per filter, summed in f64 with exact twiddle arguments.  ntaps <= N/2. */
PDSP_API int pdsp_fir_spectrum_f32(const pdsp_plan *plan, const float *taps, long long ntaps,
                                   float *h_re, float *h_im, pdsp_stream stream);
PDSP_API int pdsp_fir_spectrum_f64(const pdsp_plan *plan, const double *taps, long long ntaps,
                                   double *h_re, double *h_im, pdsp_stream stream);
/* y[r][i] = sum_j taps[j] * x[r][y_off + i - j], x zero outside [0, len), for 0 <= i < y_len and
 * rows r < batch at strides x_stride / y_stride (device pointers, any alignment); h_re / h_im from
 * pdsp_fir_spectrum_* of the same plan and ntaps.  y_off + y_len <= len + ntaps - 1; y_stride >= y_len
 * when batch > 1; y must not overlap x: a y whose byte extent ((batch - 1) * y_stride + y_len elements)
 * meets that of x gives PDSP_ERR_BAD_ARG before any launch.  8-byte aligned rows with even strides and an even y_off take
 * the 8-byte load / store path (an even ntaps runs with one zero tap more, so that hop is even). */
PDSP_API int pdsp_fir_filter_f32(const pdsp_plan *plan, long long batch, const float *x, long long len,
                                 long long x_stride, const float *h_re, const float *h_im, long long ntaps,
                                 long long y_off, long long y_len, float *y, long long y_stride,
                                 pdsp_stream stream);
PDSP_API int pdsp_fir_filter_f64(const pdsp_plan *plan, long long batch, const double *x, long long len,
                                 long long x_stride, const double *h_re, const double *h_im, long long ntaps,
                                 long long y_off, long long y_len, double *y, long long y_stride,
                                 pdsp_stream stream);

typedef enum pdsp_fir_mode {    /* output range, counted in the full convolution; m = min(len, ntaps) */
  PDSP_FIR_FULL = 0,            /* numpy.convolve "full":  offset 0,         length len + ntaps - 1 */
  PDSP_FIR_SAME = 1,            /* numpy.convolve "same":  offset (m-1)/2,   length max(len, ntaps) */
  PDSP_FIR_VALID = 2,           /* numpy.convolve "valid": offset m - 1,     length |len - ntaps| + 1 */
  PDSP_FIR_FILTER = 3           /* scipy.signal.lfilter(taps, 1, x): offset 0, length len */
} pdsp_fir_mode;
/* (y_off, y_len) of a mode for a signal of len >= 1 samples and ntaps >= 1 taps (no device work). */
PDSP_API int pdsp_fir_output_range(long long len, long long ntaps, int mode, long long *y_off,
                                   long long *y_len);
/* The block size N the host form uses for ntaps taps (1 ... 8192; 0 outside): the smallest power of
 * two >= 8 * ntaps, at least 4096 and at most 16384 ("FIR filtering"). */
PDSP_API long long pdsp_fir_block_size(long long ntaps);
/* Host f64 drop-in form (synchronous, f64 arithmetic): `batch` contiguous rows of len >= 1 samples
 * filtered by ntaps <= 8192 taps; y receives batch rows of the mode's length (pdsp_fir_output_range). */
PDSP_API int pdsp_fir_filter_host_f64(const double *x, long long batch, long long len, const double *taps,
                                      long long ntaps, int mode, double *y);

/* ---- short-time transform (complex bins) and its overlap-add inverse, f32 / f64 -------------- */
/* The reference's roadmap "A) STFT" (ROADMAP.md: pragma-dsp/xform/stft, stft(signal, opts) with complex output),
 * and the way back to the time domain.  N = pdsp_plan_size(), 64 <= N <= 16384 in both precisions (any other
 * power of two: PDSP_ERR_UNSUPPORTED_SIZE); window = NULL (rect), a plan table (pdsp_plan_window_*) or any N device
 * values.  Every argument is checked before any device work: a null plan or buffer, frames < 1, hop < 1, extents
 * that overflow 64 bits or a grid of 2^31 frames give PDSP_ERR_BAD_ARG, and so does an output whose byte extent
 * meets an input's (or the other output plane's). */

/* X_b[k] = sum_{n < N} w[n] x_b[n] e^{-2 pi i k n / N}, k = 0 ... N/2, unscaled (numpy.fft.rfft(w * frame)):
 * the framing of pdsp_spectrum_f32 -- `batch` frames at frame_stride, the first min(frame_len, N) samples used, zero
 * beyond; frame_stride = hop < frame_len reads overlapping frames of one signal in place.  re_out / im_out:
 * [batch][N/2 + 1] each.  One launch, the packed-real forward + Hermitian split; f32 ~1e-7 * sqrt(log2 N) of
 * max|X|, f64 ~1e-16. */
PDSP_API int pdsp_stft_complex_f32(const pdsp_plan *plan, long long batch, const float *frames,
                                   long long frame_len, long long frame_stride, const float *window,
                                   float *re_out, float *im_out, pdsp_stream stream);
PDSP_API int pdsp_stft_complex_f64(const pdsp_plan *plan, long long batch, const double *frames,
                                   long long frame_len, long long frame_stride, const double *window,
                                   double *re_out, double *im_out, pdsp_stream stream);
/* Weighted overlap-add inverse of `frames` >= 1 rows of N/2 + 1 bins (re_in / im_in [frames][N/2 + 1]):
 * y_b = irfft(X_b, N) (1/N; the imaginary parts of bins 0 and N/2 ignored), out has T = (frames - 1) hop + N samples,
 *   out[t] = sum_b w[t - b hop] y_b[t - b hop] / sum_b w[t - b hop]^2   over the frames covering t, ascending b,
 * and 0 where the denominator is <= 1e-11 (ends of the symmetric Hann, the gaps of hop > N).  This is
 * torch.istft(center=False, onesided=True) wherever its NOLA check passes.  hop >= N: one launch, no scratch;
 * hop < N: a frame pass into stream-ordered scratch and a gather pass per chunk of S frames, K = ceil(N/hop) - 1
 * frames recomputed per chunk, scratch min(S + K, frames) rows of N values, S = max(K + 1, 2^28 bytes / (N sizeof T)
 * - K): at most max(256 MiB, (2K + 1) N sizeof T) whatever `frames` is (256 MiB for hop >= N/64 up to N = 16384).  No atomics: bit-identical results from call to call
 * and for every chunk size.  f32 ~1e-7 * log2 N of max|y|, f64 ~1e-16 * log2 N (relative to the frames' scale). */
PDSP_API int pdsp_istft_f32(const pdsp_plan *plan, long long frames, const float *re_in, const float *im_in,
                            long long hop, const float *window, float *out, pdsp_stream stream);
PDSP_API int pdsp_istft_f64(const pdsp_plan *plan, long long frames, const double *re_in, const double *im_in,
                            long long hop, const double *window, double *out, pdsp_stream stream);
/* Host f64 forms (synchronous, f64 arithmetic, window_type a pdsp_window): signal of len >= fft_size samples
 * (PDSP_ERR_INPUT_LENGTH otherwise), F = 1 + (len - fft_size) / hop frames (the tail shorter than a hop is
 * ignored); re_out / im_out [F][fft_size/2 + 1]. */
PDSP_API int pdsp_stft_host_f64(const double *signal, long long len, long long fft_size, long long hop,
                                int window_type, double *re_out, double *im_out);
/* out: (frames - 1) hop + fft_size samples, as pdsp_istft_f64. */
PDSP_API int pdsp_istft_host_f64(const double *re, const double *im, long long frames, long long fft_size,
                                 long long hop, int window_type, double *out);

/* ---- discrete cosine transform, types 2 and 3, f32 / f64 ------------------------------------- */
/* The reference's roadmap v0.3 (ROADMAP.md: pragma-dsp/xform/dct, dct(signal, { type }), idct(...)).  Conventions
 * are scipy.fft.dct's:
 *   type 2:  y[k] = 2 sum_n x[n] cos(pi k (2n + 1) / (2N))
 *   type 3:  y[k] = x[0] + 2 sum_{n >= 1} x[n] cos(pi n (2k + 1) / (2N))
 * norm BACKWARD scales by 1, FORWARD by 1/(2N), ORTHO makes the transform orthonormal (type 2: y[0] / sqrt(4N),
 * y[k] / sqrt(2N); type 3: the backward transform of x[0] / sqrt(N), x[n] / sqrt(2N)).  The inverses follow:
 * scipy.fft.idct(x, type t, norm n) == dct(x, type 5 - t, norm n with BACKWARD and FORWARD exchanged).
 * N = pdsp_plan_size(), 64 <= N <= 16384 in both precisions (any other power of two: PDSP_ERR_UNSUPPORTED_SIZE).
 * One launch, N values in and N values out per row; f32 ~1e-7 * log2 N of max|y|, f64 ~1e-16 * log2 N.
 * Every argument is checked before any device work: a null plan or buffer, batch < 1, a stride < N, a type other
 * than 2 or 3, an unknown norm, extents that overflow 64 bits or a grid of 2^31 rows give PDSP_ERR_BAD_ARG, and so
 * does an output whose byte extent meets the input's, except the exact in-place call y == x, y_stride == x_stride. */
typedef enum pdsp_dct_norm { PDSP_DCT_BACKWARD = 0, PDSP_DCT_ORTHO = 1, PDSP_DCT_FORWARD = 2 } pdsp_dct_norm;
/* y = scipy.fft.dct(x, type, norm) per row; `batch` rows at x_stride / y_stride >= N elements */
PDSP_API int pdsp_dct_f32(const pdsp_plan *plan, long long batch, const float *x, long long x_stride, int type,
                          int norm, float *y, long long y_stride, pdsp_stream stream);
PDSP_API int pdsp_dct_f64(const pdsp_plan *plan, long long batch, const double *x, long long x_stride, int type,
                          int norm, double *y, long long y_stride, pdsp_stream stream);
/* synchronous f64 host form: `batch` contiguous rows of n values (n a power of two, 64 ... 16384) */
PDSP_API int pdsp_dct_host_f64(const double *x, long long batch, long long n, int type, int norm, double *y);

/* ---- Hilbert transform, analytic signal, envelope and instantaneous phase, f32 / f64 ----------- */
/* The reference's roadmap v0.3 ("Hilbert / analytic signal helpers").  Conventions are scipy.signal.hilbert's for an
 * even length: with X = rfft(x) of a real row of N samples,
 *   Hx = irfft(Y, N),  Y[k] = -i X[k] for 0 < k < N/2,  Y[0] = Y[N/2] = 0,   a = x + i Hx == scipy.signal.hilbert(x).
 * A row holds `len` samples, 1 <= len <= N, and is zero-padded to N (scipy.signal.hilbert(x, N=n)); every output row
 * has N samples.  out_mode selects what one launch writes per row:
 *   ANALYTIC  x[n], Hx[n] interleaved, 2N values (the real parts are the loaded samples bit for bit)
 *   IMAG      Hx[n]     ENVELOPE  |x[n] + i Hx[n]|           PHASE  atan2(Hx[n], x[n])        N values each
 * The f64 envelope is range-safe like abs(scipy.signal.hilbert(x)), a hypot: both parts are scaled by a power of two
 * before they are squared, over the whole range of f64 (so are the host form and everything built on it).  The f32
 * envelope squares in f32 (no hypot), as the f32 magnitude does: it holds its bound for samples with
 * 1.1e-19 <= |a| <= 1.8e19; above, x^2 + Hx^2 overflows, below, the squares are subnormal and then zero.
 * N = pdsp_plan_size(), 64 <= N <= 16384 in both precisions (any other power of two: PDSP_ERR_UNSUPPORTED_SIZE).
 * f32 ~1e-7 * log2 N of max|a|, f64 ~1.6e-16 * log2 N.
 * Every argument is checked before any device work: a null plan or buffer, batch < 1, len outside 1 ... N,
 * x_stride < len, y_stride < N (ANALYTIC: < 2N), an unknown out_mode, extents that overflow 64 bits or a grid of 2^31
 * rows give PDSP_ERR_BAD_ARG, and so does an output whose byte extent meets the input's, except the exact in-place
 * call y == x, y_stride == x_stride of the three N-out modes (ANALYTIC is never in place). */
typedef enum pdsp_hilbert_out {
  PDSP_HILBERT_ANALYTIC = 0,
  PDSP_HILBERT_IMAG = 1,
  PDSP_HILBERT_ENVELOPE = 2,
  PDSP_HILBERT_PHASE = 3
} pdsp_hilbert_out;
/* `batch` rows of `len` samples at x_stride elements; y rows at y_stride elements */
PDSP_API int pdsp_hilbert_f32(const pdsp_plan *plan, long long batch, const float *x, long long x_stride, long long len,
                              int out_mode, float *y, long long y_stride, pdsp_stream stream);
PDSP_API int pdsp_hilbert_f64(const pdsp_plan *plan, long long batch, const double *x, long long x_stride,
                              long long len, int out_mode, double *y, long long y_stride, pdsp_stream stream);
/* synchronous f64 host form: `batch` contiguous rows of `len` samples in, contiguous rows of n (ANALYTIC: 2n) values
 * out (n a power of two, 64 ... 16384) */
PDSP_API int pdsp_hilbert_host_f64(const double *x, long long batch, long long len, long long n, int out_mode,
                                   double *y);

/* ---- polyphase rate change: upfirdn / resample_poly, f32 / f64 -------------------------------- */
/* The reference's roadmap, "Filters and utilities": "resampling to a uniform grid", with its "windowed-sinc filter
 * design helpers".  Conventions are scipy.signal.upfirdn's and scipy.signal.resample_poly's (padtype "constant").
 * The primitive, for real rows x[0..len), real taps h[0..ntaps) and integers up, down >= 1, t0 >= 0:
 *   y[m] = sum_k h[m down + t0 - k up] x[k],   0 <= k < len, 0 <= tap index < ntaps,   m = 0 ... y_len - 1
 * -- upsample by `up` with zeros, filter, keep every `down`-th sample from t0 on -- computed in the time domain by one
 * launch that neither stores the stuffed zeros nor computes a discarded output.
 *   scipy.signal.upfirdn(h, x, up, down):   t0 = 0, y_len = ((len - 1) up + ntaps - 1) / down + 1; up, down as given.
 *   scipy.signal.resample_poly(x, up, down, window): up, down divided by their gcd, the taps times up,
 *     t0 = (ntaps - 1) / 2, y_len = ceil(len up / down); the default taps are
 *     scipy.signal.firwin(2 half + 1, 1 / max(up, down), window=("kaiser", 5.0)), half = 10 max(up, down); a window
 *     given as an array is the taps; up == down after the reduction is the identity (one tap, 1: y == x bit for bit).
 * Every output is summed over its taps in ascending order, one fma per term, so a sample's value depends on neither
 * the batch, the row's placement nor where tiles meet.  f32 ~6e-8 * T * sum|h||x| per output, T = ceil(ntaps / up)
 * (a bound, (T + 2) eps against an f64 reference); f64 the same with 2^-52.
 * Supported: 1 <= up, down <= 8192, 1 <= ntaps <= 8192 (beyond: PDSP_ERR_UNSUPPORTED_SIZE; so is a default filter of
 * more than 8192 taps, max(up, down) > 409 after the reduction), 0 <= t0 < ntaps + up, len >= 1, any y_len >= 0
 * (outputs past the data are 0), rows at strides >= their lengths.  Every argument is checked before any device work:
 * a null handle or buffer, up / down / ntaps / len < 1, a negative batch or y_len, short strides and extents that
 * overflow give PDSP_ERR_BAD_ARG, and so does a y whose byte extent ((batch - 1) * y_stride + y_len elements) meets
 * that of x. */
typedef struct pdsp_resampler pdsp_resampler;
/* The primitive: the taps as given (copied), up and down not reduced.  A resampler is tied to no FFT size; it holds
 * its taps as a phase-major table in f64, rounded once per precision and uploaded to `device` (< 0: the device
 * current at the first call) on first use.  Creation itself touches no device. */
PDSP_API int pdsp_resampler_create(int device, long long up, long long down, const double *taps, long long ntaps,
                                   long long t0, pdsp_resampler **out);
/* scipy.signal.resample_poly's set-up: the reduction by the gcd, the taps (NULL: the default design) times up, t0. */
PDSP_API int pdsp_resampler_create_poly(int device, long long up, long long down, const double *taps_or_null,
                                        long long ntaps, pdsp_resampler **out);
PDSP_API int pdsp_resampler_destroy(pdsp_resampler *rs);
/* after the reduction; the taps as convolved (resample_poly: times up), pdsp_resampler_ntaps values */
PDSP_API long long pdsp_resampler_up(const pdsp_resampler *rs);
PDSP_API long long pdsp_resampler_down(const pdsp_resampler *rs);
PDSP_API long long pdsp_resampler_ntaps(const pdsp_resampler *rs);
PDSP_API long long pdsp_resampler_t0(const pdsp_resampler *rs);
PDSP_API int pdsp_resampler_taps(const pdsp_resampler *rs, double *taps);
/* full != 0: upfirdn's ((len - 1) up + ntaps - 1) / down + 1; else resample_poly's ceil(len up / down) */
PDSP_API int pdsp_resample_output_len(const pdsp_resampler *rs, long long len, int full, long long *y_len);
/* `batch` rows of `len` samples at x_stride -> rows of y_len outputs at y_stride (device pointers, any alignment).
 * The first call of a resampler in a precision uploads its tap table (synchronously); on a stream that is being captured
 * that call is refused instead, before anything is allocated -- PDSP_ERR_BAD_ARG, "stream is capturing: ..." -- and the
 * capture stays valid: make one call outside the capture first.  The same holds for the first call of a pdsp_dwt in a
 * precision and of a pdsp_ntt. */
PDSP_API int pdsp_upfirdn_f32(const pdsp_resampler *rs, long long batch, const float *x, long long len,
                              long long x_stride, float *y, long long y_len, long long y_stride, pdsp_stream stream);
PDSP_API int pdsp_upfirdn_f64(const pdsp_resampler *rs, long long batch, const double *x, long long len,
                              long long x_stride, double *y, long long y_len, long long y_stride, pdsp_stream stream);
/* The default filter of resample_poly for up / down (reduced by their gcd first), times up: host only, no device.
 * *ntaps receives the count, 20 max(up, down) + 1 (1 when up == down); taps may be NULL to ask for the count alone. */
PDSP_API int pdsp_resample_design_f64(long long up, long long down, double *taps, long long *ntaps);
/* Host f64 drop-in forms (synchronous, f64 arithmetic): `batch` contiguous rows of len >= 1 samples in, contiguous
 * rows of ceil(len up / down) (resample_poly) or ((len - 1) up + ntaps - 1) / down + 1 (upfirdn) outputs. */
PDSP_API int pdsp_resample_poly_host_f64(const double *x, long long batch, long long len, long long up,
                                         long long down, const double *taps_or_null, long long ntaps, double *y);
PDSP_API int pdsp_upfirdn_host_f64(const double *h, long long ntaps, const double *x, long long batch, long long len,
                                   long long up, long long down, double *y);

/* ---- any-length DFT (Bluestein's chirp-z algorithm), 2 <= L <= 4096, f32 / f64 ------------------ */
/* The transform of rows whose length is NOT a power of two, with the conventions of numpy.fft.fft / numpy.fft.ifft
 * along the last axis: X[k] = sum_n x[n] exp(-2 pi i n k / L), no scaling forward, 1/L on the inverse.  Rows are
 * planar complex (re, im); a null im_in means real input (the same bits as a zero plane).  One launch per call: with
 * the chirp c[n] = exp(-i pi n^2 / L) a row becomes a circular convolution of M = max(32, the power of two >= 2L - 1)
 * points, X[k] = c[k] IFFT_M(FFT_M(x c) FFT_M(b))[k], b[j] = conj c[|j|], whose two M-point transforms run in LDS
 * (pdsp_dft_conv_size() reports M).  The chirp and FFT_M(b) / M are built in f64 on the host (n^2 reduced mod 2L in
 * integers) and rounded once per precision; they belong to the object and go to `device` (< 0: the current one) when
 * it is created.
 * Lengths: 2 <= L <= 4096, else PDSP_ERR_UNSUPPORTED_SIZE.  A power of two is accepted and takes the same kernel;
 * pdsp_plan is the fast way for those (one transform of L points instead of two of >= 2L).
 * f32 ~1e-7 * log2 M of max|X|, f64 ~1.6e-16 * log2 M (plus a few eps for the chirp products).
 * Every argument is checked before any device work: a null handle or buffer (im_in excepted), batch < 1, strides < L,
 * extents that overflow 64 bits or a grid of 2^31 rows give PDSP_ERR_BAD_ARG, and so does an output plane whose byte
 * extent meets an input plane's -- except the exact in-place call re_out == re_in, im_out == im_in, out_stride ==
 * in_stride with im_in non-null -- or the other output plane's. */
typedef struct pdsp_dft pdsp_dft;
PDSP_API int pdsp_dft_create(long long length, int device, pdsp_dft **out);
PDSP_API int pdsp_dft_destroy(pdsp_dft *d);
PDSP_API long long pdsp_dft_length(const pdsp_dft *d);
PDSP_API long long pdsp_dft_conv_size(const pdsp_dft *d);
/* `batch` rows of L points at in_stride elements -> rows of L bins at out_stride elements; inverse != 0: ifft */
PDSP_API int pdsp_dft_c2c_f32(const pdsp_dft *d, long long batch, const float *re_in, const float *im_in,
                              long long in_stride, float *re_out, float *im_out, long long out_stride, int inverse,
                              pdsp_stream stream);
PDSP_API int pdsp_dft_c2c_f64(const pdsp_dft *d, long long batch, const double *re_in, const double *im_in,
                              long long in_stride, double *re_out, double *im_out, long long out_stride, int inverse,
                              pdsp_stream stream);
/* synchronous f64 host form: `batch` contiguous rows of `length` points in (im_in NULL: real), contiguous rows out */
PDSP_API int pdsp_dft_host_f64(const double *re_in, const double *im_in, long long batch, long long length,
                               int inverse, double *re_out, double *im_out);

/* ---- chirp-z transform and zoom FFT (scipy.signal.czt / zoom_fft), f32 / f64 -------------------- */
/* K points of the z-transform of a row x of L samples, on an arc of a circle, with scipy.signal.czt's definition
 * along the last axis:
 *   X[k] = sum_{n < L} x[n] a^-n w^(n k),  k = 0 ... K - 1,   w = exp(-2 pi i step),  a = radius exp(2 pi i start)
 * i.e. the points z_k = a w^-k.  step and start are f64 numbers of TURNS (finite, below 2^53 in magnitude), radius a
 * finite f64 > 0.  Only arcs are built, |w| = 1: a spiral's chirps w^(n^2/2) span hundreds of orders of magnitude at
 * these lengths.  There is no inverse (the transform has no cheap one).  zoom_fft(fn = [f1, f2], m, fs, endpoint) is
 * step = (f2 - f1) / (fs (m - 1 if endpoint else m)), start = f1 / fs; the DFT is K = L, step = 1 / L.
 * The parameters are angles and not a complex w because the tables are the precision budget: their phases are formed
 * exactly from the doubles given.  n^2 step and n start are error-free products (p = n2 * step, e = fma(n2, step, -p)),
 * p is reduced with fmod -- mod 2 for the half-turn chirp, mod 1 for a's angle -- and e is added after the reduction,
 * so the argument of cos / sin stays below 2 pi and nothing is lost at n^2 ~ 2^26.  Note that step = 1.0 / 1000 is the
 * double NEAREST 1/1000, not 1/1000: in f64 the difference shows (about 1e-11 rad at the far corner n = k = 999);
 * pdsp_dft is the way to the exact L-th roots of unity.
 * One launch per call: with n k = (n^2 + k^2 - (k - n)^2) / 2,
 *   X[k] = post[k] sum_n (x[n] pre[n]) b[k - n]
 *   pre[n]  = a^-n w^(n^2/2)   (L entries)
 *   post[k] = w^(k^2/2)        (K entries)
 *   b[j]    = w^(-j^2/2)       for -(L - 1) <= j <= K - 1
 * a circular convolution of M = max(32, the power of two >= L + K - 1) points (pdsp_czt_conv_size() reports M) with
 * b[j] stored at index j for j >= 0, at index M + j for j < 0 and zero elsewhere, whose two M-point transforms run in
 * LDS: X[k] = post[k] IFFT_M(FFT_M(x pre) FFT_M(b))[k].  pre, post and Bt = FFT_M(b) / M are evaluated in long double
 * on the host and rounded once per precision; they belong to the object and go to `device` (< 0: the current one) when
 * it is created.
 * Limits: L >= 1, K >= 1, L + K - 1 <= 8192 (else PDSP_ERR_UNSUPPORTED_SIZE); radius^-(L-1) within [2^-64, 2^64],
 * finite step / start / radius (else PDSP_ERR_BAD_ARG).  Argument errors of pdsp_czt_create are reported before any
 * device work (device = -1 gets them on a machine without a GPU) and leave *out untouched.
 * Rows are planar complex (re, im); a null im_in means real rows (the same bits as a zero plane).
 * f32 ~1e-7 * log2 M, f64 ~1.6e-16 * log2 M (plus a few eps for the chirp products) of max(max|X|, ||x radius^-n||_2).
 * Every argument is checked before any device work: a null handle or buffer (im_in excepted), batch < 1, in_stride < L,
 * out_stride < K, extents that overflow 64 bits or a grid of 2^31 rows give PDSP_ERR_BAD_ARG.  Overlap: the exact
 * in-place call is allowed -- re_out == re_in, im_out == im_in (real rows: an im_out of its own), out_stride ==
 * in_stride (>= max(L, K) by the rule above); a workgroup loads all of its rows before its first barrier and stores
 * only into those rows.  Every other meeting of an output plane's byte extent with an input plane's, or with the other
 * output plane's, is PDSP_ERR_BAD_ARG. */
typedef struct pdsp_czt pdsp_czt;
PDSP_API int pdsp_czt_create(long long length, long long bins, double step, double start, double radius, int device,
                             pdsp_czt **out);
PDSP_API int pdsp_czt_destroy(pdsp_czt *c);
PDSP_API long long pdsp_czt_length(const pdsp_czt *c);
PDSP_API long long pdsp_czt_bins(const pdsp_czt *c);
PDSP_API long long pdsp_czt_conv_size(const pdsp_czt *c);
/* `batch` rows of L samples at in_stride elements -> rows of K points at out_stride elements */
PDSP_API int pdsp_czt_f32(const pdsp_czt *c, long long batch, const float *re_in, const float *im_in,
                          long long in_stride, float *re_out, float *im_out, long long out_stride, pdsp_stream stream);
PDSP_API int pdsp_czt_f64(const pdsp_czt *c, long long batch, const double *re_in, const double *im_in,
                          long long in_stride, double *re_out, double *im_out, long long out_stride,
                          pdsp_stream stream);
/* synchronous f64 host form: `batch` contiguous rows of `length` samples in (im_in NULL: real), contiguous rows of
 * `bins` points out */
PDSP_API int pdsp_czt_host_f64(const double *re_in, const double *im_in, long long batch, long long length,
                               long long bins, double step, double start, double radius, double *re_out,
                               double *im_out);

/* ---- multi-level discrete wavelet transform (wavedec / waverec), orthogonal filters, f32 / f64 -- */
/* h is a scaling filter of even length F, 2 <= F <= 32, and g[j] = (-1)^j h[F - 1 - j].  The extension is periodic, so
 * a row of n samples has exactly n coefficients.  One analysis level on a row a of even length m:
 *   cA[k] = sum_{j < F} h[j] a[(2k + j) mod m],   cD[k] = sum_{j < F} g[j] a[(2k + j) mod m],   0 <= k < m / 2
 * (j ascending, one fma per term from +0).  The forward transform of J levels writes the Mallat layout
 * [cA_J | cD_J | cD_{J-1} | ... | cD_1] into one row of n; n must be a positive multiple of 2^J (not a power of two:
 * 96 with J = 5 is legal), and F may exceed a level's length (the index wraps more than once).  The inverse of a level
 * is the transpose, for the output pair (2i, 2i + 1) with m' = m / 2:
 *   x[2i]     = sum_{t < F/2} ( h[2t]     cA[(i - t) mod m'] + g[2t]     cD[(i - t) mod m'] )
 *   x[2i + 1] = sum_{t < F/2} ( h[2t + 1] cA[(i - t) mod m'] + g[2t + 1] cD[(i - t) mod m'] )
 * (t ascending, the cA term before the cD term, fma from +0).  A value's bits depend on the taps and the samples
 * alone, not on the path, the tile, the batch or the stride.
 * Wavelets: the names "haar" (= "db1") and "db2" ... "db10" -- Daubechies' extremal-phase filters, sum h = sqrt 2,
 * db2 = [(1 + sqrt 3), (3 + sqrt 3), (3 - sqrt 3), (1 - sqrt 3)] / (4 sqrt 2) -- or the caller's own taps (name NULL),
 * accepted only if |sum_k h[k] h[k + 2m] - delta_m| <= 1e-10 for every m (the inverse is the transpose only then);
 * anything else is PDSP_ERR_BAD_ARG.  The taps are rounded once per precision and belong to the object.
 * Every call is one launch.  A row whose levels fit one workgroup's LDS runs there whole, to any depth, and may be
 * transformed exactly in place (y == x, equal strides).  Longer rows are cut into tiles with a halo; there the forward
 * transform takes max((F - 2)(2^J - 1), 2^J) <= 32 KiB of values (8192 f32, 4096 f64; the inverse: 2^J alone), else
 * PDSP_ERR_UNSUPPORTED_SIZE -- pdsp_dwt_max_levels() reports the deepest J for a row -- and any overlap of input and
 * output is refused.  Checked before any device work: null handle or buffers, batch < 0, len not a positive multiple
 * of 2^J, strides < len, extents that overflow 64 bits, a grid beyond 2^31 - 1 tiles, overlap (PDSP_ERR_BAD_ARG). */
typedef struct pdsp_dwt pdsp_dwt;
/* device < 0: arguments are checked without a device, the object binds to the device current at its first call */
PDSP_API int pdsp_dwt_create(int device, const char *name_or_null, const double *taps_or_null, long long ntaps,
                             int levels, pdsp_dwt **out);
PDSP_API int pdsp_dwt_destroy(pdsp_dwt *w);
PDSP_API long long pdsp_dwt_ntaps(const pdsp_dwt *w);
PDSP_API int pdsp_dwt_levels(const pdsp_dwt *w);
PDSP_API int pdsp_dwt_taps(const pdsp_dwt *w, double *taps); /* h, ntaps values */
/* the taps of a built-in wavelet: *ntaps receives F; out may be NULL (query F), else holds >= 20 values */
PDSP_API int pdsp_wavelet_taps(const char *name, double *out, long long *ntaps);
/* the deepest forward transform of rows of `len` values of elem_bytes (4 or 8) with ntaps taps: the largest J with
 * len mod 2^J == 0 that pdsp_dwt_forward_* takes; 0 for arguments outside the domain.  Needs no device. */
PDSP_API int pdsp_dwt_max_levels(long long ntaps, long long len, int elem_bytes);
/* `batch` rows of len samples at x_stride elements -> rows of len coefficients at y_stride elements, and back (the
 * first call in a precision uploads the tap table: refused on a capturing stream, as pdsp_upfirdn_f32) */
PDSP_API int pdsp_dwt_forward_f32(const pdsp_dwt *w, long long batch, const float *x, long long len,
                                  long long x_stride, float *y, long long y_stride, pdsp_stream stream);
PDSP_API int pdsp_dwt_forward_f64(const pdsp_dwt *w, long long batch, const double *x, long long len,
                                  long long x_stride, double *y, long long y_stride, pdsp_stream stream);
PDSP_API int pdsp_dwt_inverse_f32(const pdsp_dwt *w, long long batch, const float *c, long long len,
                                  long long c_stride, float *x, long long x_stride, pdsp_stream stream);
PDSP_API int pdsp_dwt_inverse_f64(const pdsp_dwt *w, long long batch, const double *c, long long len,
                                  long long c_stride, double *x, long long x_stride, pdsp_stream stream);
/* synchronous f64 host forms: `batch` contiguous rows of len values in and out; name NULL: the caller's taps */
PDSP_API int pdsp_dwt_forward_host_f64(const double *x, long long batch, long long len, const char *name_or_null,
                                       const double *taps_or_null, long long ntaps, int levels, double *y);
PDSP_API int pdsp_dwt_inverse_host_f64(const double *c, long long batch, long long len, const char *name_or_null,
                                       const double *taps_or_null, long long ntaps, int levels, double *x);

/* ---- number-theoretic transform (NTT) and exact integer convolution over GF(2^64 - 2^32 + 1), uint64 ---------- */
/* Field: GF(p), p = 2^64 - 2^32 + 1 = 18446744069414584321.  An element is a uint64_t.  An input may be any 64-bit
 * pattern and is taken mod p on load (one conditional subtraction: 2^64 < 2 p); every output is canonical, in [0, p).
 * Root: omega_N = 7^((p - 1) / N) mod p for N = 2^k, k <= 32 (7 generates the multiplicative group).  omega_4 = 2^48
 * and omega_64 = 2^39: 2 has order 192 and 2^96 = -1.
 * Transforms, natural order in and out:
 *   forward  X[k] = sum_n x[n] omega_N^(n k) mod p
 *   inverse  x[n] = N^-1 sum_k X[k] omega_N^(-n k) mod p
 * Convolution: c[i] = sum_{j + l = i (mod N)} a[j] b[l] mod p for i < out_len <= N, the rows a (a_len <= N values) and
 * b (b_len <= N) zero-padded to N: the linear product when a_len + b_len - 1 <= N, the cyclic one otherwise.
 * b_stride == 0 shares one b row among all rows of a.  One launch: both forward transforms, the point-wise product and
 * the inverse run in one kernel.
 * Nothing is rounded: a result is the same 64 bits on every path, whatever the batch, the stride or the form.
 * Sizes: N = 2^k, 64 <= N <= 16384; not a power of two: PDSP_ERR_SIZE_NOT_POW2, another power of two:
 * PDSP_ERR_UNSUPPORTED_SIZE.
 * Checked before any device work (PDSP_ERR_BAD_ARG): null handle or buffers, batch < 0, lengths outside 1 ... N,
 * strides shorter than the row (b_stride 0 excepted), extents that overflow 64 bits, a grid of 2^31 workgroups, and any
 * overlap of the output with an input other than out == in (conv: out == a) with equal strides -- a thread stores the
 * positions it loaded, so that call is exact in place. */
typedef struct pdsp_ntt pdsp_ntt;
/* device < 0: arguments are checked without a device, the object binds to the device current at its first call */
PDSP_API int pdsp_ntt_create(long long n, int device, pdsp_ntt **out);
PDSP_API int pdsp_ntt_destroy(pdsp_ntt *h);
PDSP_API long long pdsp_ntt_size(const pdsp_ntt *h);
/* `batch` rows of N values at in_stride elements -> rows of N values at out_stride elements (a handle's first
 * transform or convolution uploads its root table: refused on a capturing stream, as pdsp_upfirdn_f32) */
PDSP_API int pdsp_ntt_forward_u64(const pdsp_ntt *h, long long batch, const uint64_t *in, long long in_stride,
                                  uint64_t *out, long long out_stride, pdsp_stream stream);
PDSP_API int pdsp_ntt_inverse_u64(const pdsp_ntt *h, long long batch, const uint64_t *in, long long in_stride,
                                  uint64_t *out, long long out_stride, pdsp_stream stream);
PDSP_API int pdsp_ntt_conv_u64(const pdsp_ntt *h, long long batch, const uint64_t *a, long long a_len,
                               long long a_stride, const uint64_t *b, long long b_len, long long b_stride,
                               uint64_t *out, long long out_len, long long out_stride, pdsp_stream stream);
/* out[i] = a[i] b[i] mod p, i < count; out may be a or b itself, no other overlap */
PDSP_API int pdsp_ntt_mul_u64(long long count, const uint64_t *a, const uint64_t *b, uint64_t *out,
                              pdsp_stream stream);
/* synchronous host forms: `batch` contiguous rows of n values in and out */
PDSP_API int pdsp_ntt_host_u64(const uint64_t *x, long long batch, long long n, int inverse, uint64_t *out);
/* rows a [batch, a_len] and b ([batch, b_len], or one row when b_shared != 0) -> rows [batch, out_len] of the
 * n-point convolution */
PDSP_API int pdsp_ntt_conv_host_u64(const uint64_t *a, long long a_len, const uint64_t *b, long long b_len,
                                    int b_shared, long long batch, long long n, uint64_t *out, long long out_len);
/* device-free helpers on the arithmetic the kernels use: p; omega_n (0: n is no power of two <= 2^32); a b, a^e and
 * a^-1 mod p for any 64-bit patterns (invmod of 0 mod p is 0) */
PDSP_API uint64_t pdsp_ntt_modulus(void);
PDSP_API uint64_t pdsp_ntt_root(long long n);
PDSP_API uint64_t pdsp_ntt_mulmod(uint64_t a, uint64_t b);
PDSP_API uint64_t pdsp_ntt_powmod(uint64_t a, uint64_t e);
PDSP_API uint64_t pdsp_ntt_invmod(uint64_t a);

/* ---- sliding DFT: chosen bins of a window at every hop, f32 / f64 -------------------------------- */
/* A row x has T real samples.  The handle holds a window length N, any integer in 2 <= N <= 16384 (not only powers of
 * two), a hop h >= 1, K bins b_0 ... b_{K-1} -- finite f64 numbers of CYCLES PER WINDOW, fractional, negative and >= N
 * all allowed -- and a window type, one of the four of pdsp_window_make.  For each bin j and frame m = 0 ... F - 1,
 * F = 1 + floor((T - N) / h) (T < N is PDSP_ERR_INPUT_LENGTH):
 *   Y[j][m] = sum_{n < N} w[n] x[m h + n] exp(-2 pi i b_j n / N)
 * unscaled, the phase referenced to the frame's own first sample: Y[j][m] is numpy.fft.fft(w * x[m h : m h + N])[b_j]
 * for an integer b_j, and for a power-of-two N in 64 ... 16384 and an integer b_j <= N / 2 the bin of pdsp_stft_complex
 * with frame_len = N and the same window.
 * Windows without a window pass.  The library's windows are symmetric cosine sums in 2 pi n / (N - 1), and with
 * a = (1) for rect, (.5, .5) for Hann, (.54, .46) for Hamming and (.42, .5, .08) for Blackman
 *   sum w x e^(-2 pi i b n / N) = a_0 X(b) + sum_{c >= 1} (-1)^c a_c / 2 [X(b + c N / (N - 1)) + X(b - c N / (N - 1))]
 * with X the rectangular sum, so a windowed bin is 1, 3 or 5 COMPONENTS of the rectangular sliding sum at fractional
 * bins, added in registers before the store (pdsp_sdft_components() reports the count, pdsp_sdft_window_weights() the
 * weights in table order: 0, +1, -1, +2, -2).
 * Phases are exact.  The table entry of component (b, +-c) at position i in [0, N] is exp(-2 pi i (t1 +- t2)):
 *   t1 = ((b i) mod N) / N, b i an error-free product (p = b i, e = fma(b, i, -p)), p reduced with fmod, e added
 *        after the reduction -- the rule of the CZT's tables above -- and N added where the sum is negative;
 *   t2 = ((c i) mod (N - 1)) / (N - 1), in integers;
 * cos and sin are evaluated in long double and rounded once per precision.  Integer bins get the exact N-th roots of
 * unity, and b and b + N give the same table and the same output bits.  Note that a bin of 0.1 is the double NEAREST
 * 0.1, not 1/10: it lies 5.6e-18 cycles above, which is 3.5e-17 rad at the window's end whatever N.  The tables follow
 * the double (in long double the two differ in the 17th digit; rounded to f64 one entry in sixteen lands on the
 * neighbouring value at N = 1000) -- far less than the CZT's step shows, because a bin is multiplied by n / N <= 1 and not by n k
 * (pdsp_sdft_phase_table() gives the table of one component, device-free).
 * The algorithm is parallel in time, O(K) per sample and has no drift: the row is cut into anchored chunks of N
 * samples, every frame is the suffix of one chunk's products x tab plus tab[N] times the prefix of the next chunk's,
 * and both come from scans of their own (pdsp_sdft_kernel.h states the one summation order).  A frame's value is a
 * function of its own N samples and of (m h) mod N alone: the bits do not depend on the batch, the strides, T, the
 * hop, the tiling or the other bins of the handle, a NaN or Inf reaches exactly the frames that contain it, and frame
 * 10^6 has the error of frame 0.  Error: a few u sqrt(N) max|x| in the worst case over a call, u the unit roundoff
 * (DESIGN.md 4.15 has the measured figures).
 * Limits: 1 <= K <= 256 and K components (N + 1) <= 2^21 table entries, N outside 2 ... 16384:
 * PDSP_ERR_UNSUPPORTED_SIZE; hop < 1, an unknown window, a null, non-finite or |b| >= 2^53 bin: PDSP_ERR_BAD_ARG.
 * Argument errors of pdsp_sdft_create are reported before any device work (device = -1 gets them on a machine without
 * a GPU) and leave *out untouched.  The tables belong to the object and go to `device` (< 0: the current one) when it
 * is created.
 * Launches: series (r, j) of row r and bin j starts at (r K + j) out_stride in each plane, out_stride >= F; only the F
 * values of a series are written, and nothing outside [0, T) of a row is read.  A null handle or buffer, batch < 1,
 * in_stride < T, out_stride < F, extents that overflow 64 bits, a grid of 2^31 workgroups, and any meeting of an
 * output plane's byte extent with the input's or the other output plane's (there is no in-place form) give
 * PDSP_ERR_BAD_ARG, before any device work. */
typedef struct pdsp_sdft pdsp_sdft;
PDSP_API int pdsp_sdft_create(long long window_len, long long nbins, const double *bins, long long hop,
                              int window_type, int device, pdsp_sdft **out);
PDSP_API int pdsp_sdft_destroy(pdsp_sdft *c);
PDSP_API long long pdsp_sdft_length(const pdsp_sdft *c);
PDSP_API long long pdsp_sdft_bins(const pdsp_sdft *c);
PDSP_API double pdsp_sdft_bin(const pdsp_sdft *c, long long index);
PDSP_API long long pdsp_sdft_hop(const pdsp_sdft *c);
PDSP_API long long pdsp_sdft_components(const pdsp_sdft *c);
/* F for rows of `samples` values; 0 where samples < N */
PDSP_API long long pdsp_sdft_frames(const pdsp_sdft *c, long long samples);
/* `batch` rows of `samples` values at in_stride -> per row and bin a series of F values in each plane */
PDSP_API int pdsp_sdft_f32(const pdsp_sdft *c, long long batch, const float *in, long long in_stride,
                           long long samples, float *re_out, float *im_out, long long out_stride, pdsp_stream stream);
PDSP_API int pdsp_sdft_f64(const pdsp_sdft *c, long long batch, const double *in, long long in_stride,
                           long long samples, double *re_out, double *im_out, long long out_stride,
                           pdsp_stream stream);
/* synchronous f64 host form: `batch` contiguous rows of `samples` values in, contiguous planes [batch][nbins][F] out */
PDSP_API int pdsp_sdft_host_f64(const double *in, long long batch, long long samples, long long window_len,
                                long long nbins, const double *bins, long long hop, int window_type, double *re_out,
                                double *im_out);
/* device-free: the component weights of a window in table order (returns their number, 0 for an unknown type), and
 * the window_len + 1 table entries of component c in -2 ... 2 of one bin */
PDSP_API int pdsp_sdft_window_weights(int window_type, double weights[5]);
PDSP_API int pdsp_sdft_phase_table(long long window_len, double bin, int component, double *re_out, double *im_out);

#ifdef __cplusplus
}
#endif
#endif /* PDSP_HIP_H */

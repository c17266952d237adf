/*
 * pdsp_napi.c -- Node N-API addon: the binding a pragma-dsp maintainer adds to
 * re-back src/core/fft.ts and src/xform/fourier.ts with libpdsp_hip.so.
 *
 * Thin by design: typed-array pointers in, the C ABI of include/pdsp_hip.h
 * called, status mapped to `throw new Error(pdsp_last_error())` (the reference's
 * error convention).  ArrayLike flattening (`?? 0`), `out` identity and
 * option defaults live in the JS host (pragma-dsp_amd/js/), not here.
 *
 * Native plans are wrapped in a napi external with a finalizer: the reference's
 * Radix2Fft has no destroy() method, so the GC frees the device tables.
 *
 * How a JS value becomes a C number or pointer, and what is thrown when it does not, is known by the first section
 * alone (`args` and its accessors, typed_span, collect_rows); an export reads its arguments through them, scalars
 * first and typed arrays last, and tests one flag.
 */
#include <node_api.h>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "pdsp_hip.h"

/* The size limits of include/pdsp_hip.h that the output checks below mirror: a request inside them must fit the
 * caller's arrays; one outside them goes to the library unchanged, which refuses it before it writes. */
#define PACKED_MIN 64     /* the packed-real families (STFT, Hilbert, NTT): 64 <= N <= 16384; sliding DFT: N <= 16384 */
#define PACKED_MAX 16384
#define RATIO_MAX 8192    /* resampling: up, down and taps <= 8192; chirp-z: length + bins - 1 <= 8192 */
#define DFT_MAX 4096      /* any-length DFT: 2 <= L <= 4096 */
#define SDFT_BINS_MAX 256 /* sliding DFT: 1 ... 256 bins */

/* ---- refusals ------------------------------------------------------------------------------------------------- */

static napi_value refuse(napi_env env, const char *text) {
  napi_throw_error(env, NULL, text);
  return NULL;
}

static napi_value throw_pdsp(napi_env env) { return refuse(env, pdsp_last_error()); }

/* the end of an export that returns nothing: the library's status as undefined or as its error */
static napi_value done(napi_env env, int rc) { return rc == PDSP_OK ? NULL : throw_pdsp(env); }

#define NAPI_OK_OR_THROW(env, call) \
  if ((call) != napi_ok) return refuse((env), "pdsp_napi: N-API call failed: " #call)

/* ---- typed arrays --------------------------------------------------------------------------------------------- */

typedef struct { double *p; size_t n; } f64_span;
typedef struct { uint64_t *p; size_t n; } u64_span;

/* the kinds a parameter accepts; K_NULL: null / undefined is (NULL, 0) */
enum { K_F64 = 1, K_F32 = 2, K_U64 = 4, K_NULL = 8 };

/* The one classification of a typed-array value: its kind (one of `kinds`) with data pointer and length, or 0 with a
 * TypeError thrown.  It runs no JS: a pointer read here stays valid until the next call that can. */
static int typed_span(napi_env env, napi_value v, int kinds, void **data, size_t *len) {
  napi_valuetype t;
  napi_typedarray_type tt;
  *data = NULL;
  *len = 0;
  if ((kinds & K_NULL) && napi_typeof(env, v, &t) == napi_ok && (t == napi_null || t == napi_undefined)) return K_NULL;
  int kind = 0;
  if (napi_get_typedarray_info(env, v, &tt, len, data, NULL, NULL) == napi_ok) /* else: not a typed array at all */
    kind = tt == napi_float64_array ? K_F64 : tt == napi_float32_array ? K_F32 : tt == napi_biguint64_array ? K_U64 : 0;
  if (kind & kinds) return kind;
  *data = NULL;
  *len = 0;
  napi_throw_type_error(env, NULL, (kinds & K_U64)   ? "pdsp_napi: expected a BigUint64Array"
                                   : (kinds & K_F32) ? "pdsp_napi: expected a Float64Array or a Float32Array"
                                                     : "pdsp_napi: expected a Float64Array");
  return 0;
}

/* ---- arguments ------------------------------------------------------------------------------------------------ */

/* The arguments of one call.  The first one that is not what its accessor expects throws its TypeError and clears
 * `ok`; every later accessor then returns zero, so an export reads all its arguments and tests `ok` once. */
#define MAX_ARGS 12
typedef struct {
  napi_env env;
  napi_value v[MAX_ARGS];
  int ok;
} args;

static int arg_bad(args *a, const char *text) {
  if (a->ok) napi_throw_type_error(a->env, NULL, text);
  return a->ok = 0;
}

static void args_read(args *a, napi_env env, napi_callback_info info, size_t want) {
  size_t argc = want;
  a->env = env;
  a->ok = 1;
  if (napi_get_cb_info(env, info, &argc, a->v, NULL, NULL) != napi_ok || argc < want)
    arg_bad(a, "pdsp_napi: wrong number of arguments");
}

static int64_t arg_i64(args *a, int i) {
  int64_t x = 0;
  if (a->ok && napi_get_value_int64(a->env, a->v[i], &x) != napi_ok) arg_bad(a, "pdsp_napi: expected a number");
  return a->ok ? x : 0;
}

/* An int64 that becomes a C `int` (window type, sides, mode, DCT type and norm, levels): a value outside int's range
 * is never truncated into it but becomes `refused`, a value of the parameter that the library refuses. */
static int arg_int(args *a, int i, int refused) {
  const int64_t x = arg_i64(a, i);
  return x < INT_MIN || x > INT_MAX ? refused : (int)x;
}

static double arg_f64(args *a, int i) {
  double x = 0;
  if (a->ok && napi_get_value_double(a->env, a->v[i], &x) != napi_ok) arg_bad(a, "pdsp_napi: expected a number");
  return a->ok ? x : 0;
}

static bool arg_bool(args *a, int i) {
  bool x = false;
  if (a->ok && napi_get_value_bool(a->env, a->v[i], &x) != napi_ok) arg_bad(a, "pdsp_napi: expected a boolean");
  return a->ok && x;
}

static pdsp_plan *arg_plan(args *a, int i) {
  void *p = NULL;
  if (a->ok && napi_get_value_external(a->env, a->v[i], &p) != napi_ok) arg_bad(a, "pdsp_napi: expected a plan");
  return a->ok ? (pdsp_plan *)p : NULL;
}

/* a string into buf, or NULL for null / undefined */
static const char *arg_str(args *a, int i, char *buf, size_t cap) {
  napi_valuetype t;
  size_t got = 0;
  if (!a->ok || (napi_typeof(a->env, a->v[i], &t) == napi_ok && (t == napi_null || t == napi_undefined))) return NULL;
  if (napi_get_value_string_utf8(a->env, a->v[i], buf, cap, &got) != napi_ok) arg_bad(a, "pdsp_napi: expected a string");
  return a->ok ? buf : NULL;
}

/* Float64Array -> (double*, length).  null/undefined -> (NULL, 0). */
static f64_span arg_f64s(args *a, int i) {
  f64_span s = {NULL, 0};
  if (a->ok && !typed_span(a->env, a->v[i], K_F64 | K_NULL, (void **)&s.p, &s.n)) a->ok = 0;
  return s;
}

/* BigUint64Array -> (uint64_t*, length).  null/undefined -> (NULL, 0). */
static u64_span arg_u64s(args *a, int i) {
  u64_span s = {NULL, 0};
  if (a->ok && !typed_span(a->env, a->v[i], K_U64 | K_NULL, (void **)&s.p, &s.n)) a->ok = 0;
  return s;
}

/* a JS array and its length; anything else throws `text` */
static napi_value arg_array(args *a, int i, const char *text, uint32_t *len) {
  bool is_array = false;
  *len = 0;
  if (a->ok && (napi_is_array(a->env, a->v[i], &is_array) != napi_ok || !is_array ||
                napi_get_array_length(a->env, a->v[i], len) != napi_ok))
    arg_bad(a, text);
  return a->v[i];
}

/* ---- extents -------------------------------------------------------------------------------------------------- */

/* a * b of two extents (batch * len, batch * bins, 4 * batch, rows * size, frames * bins; both >= 0), INT64_MAX where
 * the product overflows: a length no array has, so "too small" for every check that compares against it. */
static int64_t extent(int64_t a, int64_t b) {
  int64_t r;
  return __builtin_mul_overflow(a, b, &r) ? INT64_MAX : r;
}

static int holds(f64_span s, int64_t need) { return (int64_t)s.n >= need; }

static double no_samples = 0.0; /* stands in where a zero-length typed array has no data pointer */

/* ---- rows ----------------------------------------------------------------------------------------------------- */

/* Elements start .. start + count - 1 of the JS array `list` as row pointers, for transformRows and spectrumRows:
 * typed arrays of one of `kinds`, or, complex, { real, imag } pairs of them into re[] and im[]; every plane of `len`
 * values, else `len_text` is thrown.  Returns the run's kind, 0 after a throw.
 *
 * Two passes, because reading an element or a property can run user JS (an accessor-defined index, a `real` getter),
 * and that JS can detach or transfer a buffer whose pointer was read earlier.  Pass 1 fetches every value and reads
 * no pointer.  Pass 2 is typed_span alone, which runs no JS, so the pointers it reads are all valid together, up to
 * the library call.  A buffer detached during pass 1 shows up in pass 2 with length 0 and is refused by the length
 * check. */
static int collect_rows(napi_env env, napi_value list, uint32_t start, size_t count, bool complex, int kinds, size_t len,
                        const char *len_text, const void **re, const void **im) {
  const size_t per = complex ? 2 : 1;
  napi_handle_scope scope;
  napi_value *vals = (napi_value *)malloc(sizeof(napi_value) * (count ? count * per : 1));
  if (!vals || napi_open_handle_scope(env, &scope) != napi_ok) {
    free(vals);
    refuse(env, vals ? "pdsp_napi: N-API call failed: napi_open_handle_scope" : "pdsp_napi: out of memory");
    return 0;
  }
  int ok = 1, run = 0;
  for (size_t b = 0; ok && b < count; ++b) { /* pass 1: values only */
    napi_value el;
    napi_valuetype t;
    ok = napi_get_element(env, list, start + (uint32_t)b, &el) == napi_ok;
    if (ok && !complex) {
      vals[b] = el;
    } else if (ok) {
      ok = napi_typeof(env, el, &t) == napi_ok && t == napi_object;
      if (!ok) napi_throw_type_error(env, NULL, "pdsp_napi: transformRows expects { real, imag } rows");
      ok = ok && napi_get_named_property(env, el, "real", &vals[2 * b]) == napi_ok &&
           napi_get_named_property(env, el, "imag", &vals[2 * b + 1]) == napi_ok;
    }
  }
  bool pending = false;
  if (!ok && napi_is_exception_pending(env, &pending) == napi_ok && !pending)
    refuse(env, "pdsp_napi: N-API call failed while reading a row");
  for (size_t i = 0; ok && i < count * per; ++i) { /* pass 2: pointers, kinds and lengths; no JS runs from here on */
    void *p;
    size_t n;
    const int kind = typed_span(env, vals[i], kinds, &p, &n);
    if (!kind) {
      ok = 0;
    } else if (n != len) {
      refuse(env, len_text);
      ok = 0;
    } else if (run && kind != run) {
      napi_throw_type_error(env, NULL, "pdsp_napi: spectrumRows frames must all be of one typed-array kind");
      ok = 0;
    }
    run = kind;
    (complex && (i & 1) ? im : re)[i / per] = p ? p : (void *)&no_samples;
  }
  napi_close_handle_scope(env, scope);
  free(vals);
  return ok ? (run ? run : K_F64) : 0;
}

/* ---- plans and transforms ------------------------------------------------------------------------------------- */

static void plan_finalize(napi_env env, void *data, void *hint) {
  (void)env;
  (void)hint;
  pdsp_plan_destroy((pdsp_plan *)data);
}

/* planCreate(size) -> external   [new Radix2Fft(size), src/core/fft.ts:68-75] */
static napi_value PlanCreate(napi_env env, napi_callback_info info) {
  args a;
  args_read(&a, env, info, 1);
  const int64_t size = arg_i64(&a, 0);
  if (!a.ok) return NULL;
  pdsp_plan *plan = NULL;
  if (pdsp_plan_create(size, -1, &plan) != PDSP_OK) return throw_pdsp(env);
  napi_value ext;
  NAPI_OK_OR_THROW(env, napi_create_external(env, plan, plan_finalize, NULL, &ext));
  return ext;
}

/* transform(plan, re, imOrNull, outRe, outIm, inverse)   [Radix2Fft.transform, fft.ts:89-151] */
static napi_value Transform(napi_env env, napi_callback_info info) {
  args a;
  args_read(&a, env, info, 6);
  pdsp_plan *plan = arg_plan(&a, 0);
  const bool inverse = arg_bool(&a, 5);
  const f64_span re = arg_f64s(&a, 1), im = arg_f64s(&a, 2), ore = arg_f64s(&a, 3), oim = arg_f64s(&a, 4);
  if (!a.ok) return NULL;
  const long long n = pdsp_plan_size(plan);
  /* the length checks of fft.ts:95-104, real plane first, then imaginary */
  const long long bad = (long long)re.n != n ? (long long)re.n : im.p && (long long)im.n != n ? (long long)im.n : -1;
  if (bad >= 0) {
    char msg[128];
    snprintf(msg, sizeof(msg), "FFT input length %lld != size %lld", bad, n);
    return refuse(env, msg);
  }
  if ((long long)ore.n != n || (long long)oim.n != n)
    return refuse(env, "pdsp_napi: output planes must have the plan's size");
  return done(env, pdsp_fft_transform_host_f64(plan, 1, n, re.p, im.p, ore.p, oim.p, inverse));
}

/* transformBatch(plan, batch, re, imOrNull, outRe, outIm, inverse): `batch` rows of the plan's size, planes of
 * batch*size values   [Radix2Fft.transform row by row, fft.ts:89-151; the loop of bench/reallife/signals.ts:264-270
 * as one call] */
static napi_value TransformBatch(napi_env env, napi_callback_info info) {
  args a;
  args_read(&a, env, info, 7);
  pdsp_plan *plan = arg_plan(&a, 0);
  const int64_t batch = arg_i64(&a, 1);
  const bool inverse = arg_bool(&a, 6);
  const f64_span re = arg_f64s(&a, 2), im = arg_f64s(&a, 3), ore = arg_f64s(&a, 4), oim = arg_f64s(&a, 5);
  if (!a.ok) return NULL;
  const long long n = pdsp_plan_size(plan);
  if (batch < 0 || n <= 0 || batch > (int64_t)(((size_t)-1) / 16 / (size_t)n))
    return refuse(env, "pdsp_napi: transformBatch bad batch");
  const size_t want = (size_t)extent(batch, n);
  if (re.n != want || (im.p && im.n != want) || ore.n != want || oim.n != want)
    return refuse(env, "pdsp_napi: transformBatch planes must hold batch * size values");
  if (inverse && !im.p && batch > 0) return refuse(env, "pdsp_napi: transformBatch inverse needs an imaginary plane");
  return done(env, pdsp_fft_transform_host_f64(plan, batch, n, re.p, im.p, ore.p, oim.p, inverse));
}

/* transformRows(plan, inputs, complex, outRe, outIm, inverse): inputs is a JS array of Float64Arrays (complex =
 * false: real rows) or of { real, imag } pairs of Float64Arrays, every plane of the plan's size -- read where they
 * lie (pdsp_fft_transform_rows_host_f64); outRe / outIm hold inputs.length * size values. */
static napi_value TransformRows(napi_env env, napi_callback_info info) {
  args a;
  uint32_t batch;
  args_read(&a, env, info, 6);
  pdsp_plan *plan = arg_plan(&a, 0);
  const napi_value inputs = arg_array(&a, 1, "pdsp_napi: transformRows expects an array of rows", &batch);
  const bool complex = arg_bool(&a, 2), inverse = arg_bool(&a, 5);
  const f64_span ore = arg_f64s(&a, 3), oim = arg_f64s(&a, 4);
  if (!a.ok) return NULL;
  const long long n = pdsp_plan_size(plan);
  const int64_t want = extent(batch, n);
  if (n <= 0 || (int64_t)ore.n != want || (int64_t)oim.n != want)
    return refuse(env, "pdsp_napi: transformRows output planes must hold rows * size values");
  if (inverse && !complex && batch > 0) return refuse(env, "pdsp_napi: transformRows inverse needs complex rows");
  const void **re = (const void **)malloc(sizeof(void *) * 2 * (size_t)(batch ? batch : 1));
  if (!re) return refuse(env, "pdsp_napi: out of memory");
  const void **im = complex ? re + batch : NULL; /* one block: the real rows' pointers, then the imaginary rows' */
  int rc = PDSP_OK;                              /* stays so after a refused row: its error is already pending */
  /* a null row or plane passes the classification as (NULL, 0) and is refused by the length check */
  if (collect_rows(env, inputs, 0, batch, complex, K_F64 | K_NULL, (size_t)n,
                   "pdsp_napi: transformRows rows must be Float64Arrays of the plan's size", re, im))
    rc = pdsp_fft_transform_rows_host_f64(plan, (long long)batch, n, (const double *const *)re,
                                          (const double *const *)im, ore.p, oim.p, inverse);
  free(re);
  return done(env, rc);
}

/* ---- windows and element-wise helpers ------------------------------------------------------------------------- */

/* windowMake(type, size, out)   [createWindow, fourier.ts:14-52] */
static napi_value WindowMake(napi_env env, napi_callback_info info) {
  args a;
  args_read(&a, env, info, 3);
  const int type = arg_int(&a, 0, -1);
  const int64_t size = arg_i64(&a, 1);
  const f64_span out = arg_f64s(&a, 2);
  if (!a.ok) return NULL;
  if (!holds(out, size)) return refuse(env, "pdsp_napi: window output too small");
  return done(env, pdsp_window_make(type, size, out.p));
}

/* applyWindow(in, win, out)   [fourier.ts:54-67] */
static napi_value ApplyWindow(napi_env env, napi_callback_info info) {
  args a;
  args_read(&a, env, info, 3);
  const f64_span in = arg_f64s(&a, 0), win = arg_f64s(&a, 1), out = arg_f64s(&a, 2);
  if (!a.ok) return NULL;
  if (out.n < in.n && in.n == win.n) return refuse(env, "pdsp_napi: applyWindow output too small");
  return done(env, pdsp_apply_window_host_f64(in.p, (long long)in.n, win.p, (long long)win.n, out.p));
}

static napi_value polar(napi_env env, napi_callback_info info, int want_phase) {
  args a;
  args_read(&a, env, info, 3);
  const f64_span re = arg_f64s(&a, 0), im = arg_f64s(&a, 1), out = arg_f64s(&a, 2);
  if (!a.ok) return NULL;
  if (im.n < re.n || out.n < re.n) return refuse(env, "pdsp_napi: magnitude/phase planes too small");
  const int rc = want_phase ? pdsp_phase_host_f64(re.p, im.p, (long long)re.n, out.p)
                            : pdsp_magnitude_host_f64(re.p, im.p, (long long)re.n, out.p);
  return done(env, rc);
}
/* magnitude(re, im, out) / phase(re, im, out)   [fourier.ts:98-120] */
static napi_value Magnitude(napi_env env, napi_callback_info info) { return polar(env, info, 0); }
static napi_value Phase(napi_env env, napi_callback_info info) { return polar(env, info, 1); }

/* ---- spectra -------------------------------------------------------------------------------------------------- */

/* The spectrum outputs fit: freq holds bins values, amp and phase batch * bins, peaks (where the export has them)
 * 4 * batch, for bins = size / 2 + 1 one-sided, else size.  A size that is no power of two passes: the library refuses
 * it before it writes, with the reference's text. */
static int spectrum_outputs_fit(int64_t fft_size, int64_t len, int sides, int64_t batch, f64_span freq, f64_span amp,
                                f64_span ph, const f64_span *peaks) {
  const long long n = fft_size >= 0 ? fft_size : pdsp_next_pow2((long long)len);
  const int64_t bins = sides == PDSP_SIDES_ONE ? n / 2 + 1 : n;
  if (!pdsp_is_pow2(n)) return 1;
  return holds(freq, bins) && holds(amp, extent(batch, bins)) && holds(ph, extent(batch, bins)) &&
         (!peaks || holds(*peaks, extent(4, batch)));
}

/* peak records into 4 doubles per frame: index, frequency, amplitude, phase */
static void peaks_to_f64(const pdsp_peak *recs, int64_t batch, double *pk) {
  for (int64_t b = 0; b < batch; ++b) {
    pk[4 * b + 0] = (double)recs[b].index;
    pk[4 * b + 1] = recs[b].frequency;
    pk[4 * b + 2] = recs[b].amplitude;
    pk[4 * b + 3] = recs[b].phase;
  }
}

/* spectrum(samples, sampleRate, fftSizeOrMinus1, window, sides, freq, amp, phase) -> peak
 * [spectrum(), src/public/spectrum.ts:107-142] */
static napi_value Spectrum(napi_env env, napi_callback_info info) {
  args a;
  args_read(&a, env, info, 8);
  const double rate = arg_f64(&a, 1);
  const int64_t fft_size = arg_i64(&a, 2);
  const int window = arg_int(&a, 3, -1), sides = arg_int(&a, 4, -1);
  const f64_span x = arg_f64s(&a, 0), freq = arg_f64s(&a, 5), amp = arg_f64s(&a, 6), ph = arg_f64s(&a, 7);
  if (!a.ok) return NULL;
  if (!spectrum_outputs_fit(fft_size, (int64_t)x.n, sides, 1, freq, amp, ph, NULL))
    return refuse(env, "pdsp_napi: spectrum outputs too small");
  pdsp_peak pk;
  long long got = 0;
  if (pdsp_spectrum_host_f64(x.n ? x.p : &no_samples, (long long)x.n, rate, fft_size, window, sides, freq.p, amp.p, ph.p,
                             &pk, &got) != PDSP_OK)
    return throw_pdsp(env);
  napi_value obj, v;
  NAPI_OK_OR_THROW(env, napi_create_object(env, &obj));
  NAPI_OK_OR_THROW(env, napi_create_int32(env, pk.index, &v));
  NAPI_OK_OR_THROW(env, napi_set_named_property(env, obj, "index", v));
  NAPI_OK_OR_THROW(env, napi_create_double(env, pk.frequency, &v));
  NAPI_OK_OR_THROW(env, napi_set_named_property(env, obj, "frequency", v));
  NAPI_OK_OR_THROW(env, napi_create_double(env, pk.amplitude, &v));
  NAPI_OK_OR_THROW(env, napi_set_named_property(env, obj, "amplitude", v));
  NAPI_OK_OR_THROW(env, napi_create_double(env, pk.phase, &v));
  NAPI_OK_OR_THROW(env, napi_set_named_property(env, obj, "phase", v));
  return obj;
}

/* spectrumBatch(frames, batch, frameLen, sampleRate, fftSizeOrMinus1, window, sides, freq, amp, phase, peaks)
 * frames: batch*frameLen samples; amp/phase: batch*bins; peaks: 4 doubles per frame
 * (index, frequency, amplitude, phase)   [the map of spectrumStream, src/effect/index.ts:190-194] */
static napi_value SpectrumBatch(napi_env env, napi_callback_info info) {
  args a;
  args_read(&a, env, info, 11);
  const int64_t batch = arg_i64(&a, 1), len = arg_i64(&a, 2);
  const double rate = arg_f64(&a, 3);
  const int64_t fft_size = arg_i64(&a, 4);
  const int window = arg_int(&a, 5, -1), sides = arg_int(&a, 6, -1);
  const f64_span x = arg_f64s(&a, 0), freq = arg_f64s(&a, 7), amp = arg_f64s(&a, 8), ph = arg_f64s(&a, 9),
                 pk = arg_f64s(&a, 10);
  if (!a.ok) return NULL;
  if (batch < 0 || len < 0 || !holds(x, extent(batch, len)))
    return refuse(env, "pdsp_napi: spectrumBatch frames buffer too small");
  if (!spectrum_outputs_fit(fft_size, len, sides, batch, freq, amp, ph, &pk))
    return refuse(env, "pdsp_napi: spectrumBatch outputs too small");
  pdsp_peak *recs = (pdsp_peak *)malloc(sizeof(pdsp_peak) * (size_t)(batch > 0 ? batch : 1));
  if (!recs) return refuse(env, "pdsp_napi: out of memory");
  const int rc = pdsp_spectrum_batch_host_f64(x.n ? x.p : &no_samples, batch, len, rate, fft_size, window, sides, freq.p,
                                              amp.p, ph.p, recs, NULL);
  if (rc == PDSP_OK) peaks_to_f64(recs, batch, pk.p);
  free(recs);
  return done(env, rc);
}

/* spectrumRows(frames, start, batch, frameLen, sampleRate, fftSizeOrMinus1, window, sides, freq, amp, phase, peaks)
 * frames: a JS array whose elements start .. start+batch-1 are all Float64Arrays or all Float32Arrays of frameLen
 * samples each -- taken where they lie (pdsp_spectrum_rows_host_f64 / _f32in), not flattened; outputs as
 * spectrumBatch. */
static napi_value SpectrumRows(napi_env env, napi_callback_info info) {
  args a;
  uint32_t nframes;
  args_read(&a, env, info, 12);
  const napi_value frames = arg_array(&a, 0, "pdsp_napi: spectrumRows expects an array of Float64Arrays", &nframes);
  const int64_t start = arg_i64(&a, 1), batch = arg_i64(&a, 2), len = arg_i64(&a, 3);
  const double rate = arg_f64(&a, 4);
  const int64_t fft_size = arg_i64(&a, 5);
  const int window = arg_int(&a, 6, -1), sides = arg_int(&a, 7, -1);
  const f64_span freq = arg_f64s(&a, 8), amp = arg_f64s(&a, 9), ph = arg_f64s(&a, 10), pk = arg_f64s(&a, 11);
  if (!a.ok) return NULL;
  if (start < 0 || batch < 0 || len < 0 || start > (int64_t)nframes || batch > (int64_t)nframes - start)
    return refuse(env, "pdsp_napi: spectrumRows frame range out of bounds");
  if (!spectrum_outputs_fit(fft_size, len, sides, batch, freq, amp, ph, &pk))
    return refuse(env, "pdsp_napi: spectrumRows outputs too small");
  const void **rows = (const void **)malloc(sizeof(void *) * (size_t)(batch > 0 ? batch : 1));
  pdsp_peak *recs = (pdsp_peak *)malloc(sizeof(pdsp_peak) * (size_t)(batch > 0 ? batch : 1));
  int rc = PDSP_OK; /* stays so after a refused frame: its error is already pending */
  if (!rows || !recs) {
    refuse(env, "pdsp_napi: out of memory");
  } else {
    /* the run's element type: every frame a Float64Array, or every frame a Float32Array */
    const int kind = collect_rows(env, frames, (uint32_t)start, (size_t)batch, false, K_F64 | K_F32, (size_t)len,
                                  "pdsp_napi: spectrumRows frames must all have frameLen samples", rows, NULL);
    if (kind == K_F32)
      rc = pdsp_spectrum_rows_host_f32in((const float *const *)rows, batch, len, rate, fft_size, window, sides, freq.p,
                                         amp.p, ph.p, recs, NULL);
    else if (kind)
      rc = pdsp_spectrum_rows_host_f64((const double *const *)rows, batch, len, rate, fft_size, window, sides, freq.p,
                                       amp.p, ph.p, recs, NULL);
    if (kind && rc == PDSP_OK) peaks_to_f64(recs, batch, pk.p);
  }
  free(rows);
  free(recs);
  return done(env, rc);
}

/* binFrequencies(size, sampleRate, sides, out)   [fourier.ts:147-165] */
static napi_value BinFrequencies(napi_env env, napi_callback_info info) {
  args a;
  args_read(&a, env, info, 4);
  const int64_t size = arg_i64(&a, 0);
  const double rate = arg_f64(&a, 1);
  const int sides = arg_int(&a, 2, -1);
  const f64_span out = arg_f64s(&a, 3);
  if (!a.ok) return NULL;
  /* size / rate errors keep the reference's texts (the C call validates before it writes); a valid request must
   * fit the caller's array: size/2 + 1 values one-sided, size two-sided */
  if (size > 0 && rate > 0 && !holds(out, sides == PDSP_SIDES_ONE ? size / 2 + 1 : size))
    return refuse(env, "pdsp_napi: binFrequencies output too small");
  return done(env, pdsp_bin_frequencies(size, rate, sides, out.p, NULL));
}

/* fftShift(in, out)   [fourier.ts:122-134] */
static napi_value FftShift(napi_env env, napi_callback_info info) {
  args a;
  args_read(&a, env, info, 2);
  const f64_span in = arg_f64s(&a, 0), out = arg_f64s(&a, 1);
  if (!a.ok) return NULL;
  if (out.n < in.n) return refuse(env, "pdsp_napi: fftShift output too small");
  return done(env, pdsp_fft_shift_f64(in.p, (long long)in.n, out.p));
}

static napi_value NextPow2(napi_env env, napi_callback_info info) {
  args a;
  napi_value out;
  args_read(&a, env, info, 1);
  const int64_t n = arg_i64(&a, 0);
  if (!a.ok) return NULL;
  NAPI_OK_OR_THROW(env, napi_create_int64(env, pdsp_next_pow2(n), &out));
  return out;
}

static napi_value DeviceCount(napi_env env, napi_callback_info info) {
  (void)info;
  napi_value out;
  NAPI_OK_OR_THROW(env, napi_create_int32(env, pdsp_device_count(), &out));
  return out;
}

/* ---- filters and rate change ---------------------------------------------------------------------------------- */

/* firFilter(signal, taps, mode, out) -> out holds the mode's outputs (pdsp_fir_output_range)
 * [pragma-dsp/filters of ROADMAP.md, "Filters and utilities"; include/pdsp_hip.h, "FIR filtering"] */
static napi_value FirFilter(napi_env env, napi_callback_info info) {
  args a;
  args_read(&a, env, info, 4);
  const int mode = arg_int(&a, 2, -1);
  const f64_span x = arg_f64s(&a, 0), h = arg_f64s(&a, 1), y = arg_f64s(&a, 3);
  if (!a.ok) return NULL;
  long long y_off = 0, y_len = 0;
  if (pdsp_fir_output_range((long long)x.n, (long long)h.n, mode, &y_off, &y_len) != PDSP_OK) return throw_pdsp(env);
  if (!holds(y, y_len)) return refuse(env, "pdsp_napi: firFilter output too small");
  return done(env, pdsp_fir_filter_host_f64(x.p, 1, (long long)x.n, h.p, (long long)h.n, mode, y.p));
}

static int ratio_ok(int64_t up, int64_t down) { return up >= 1 && up <= RATIO_MAX && down >= 1 && down <= RATIO_MAX; }

/* resamplePoly(signal, up, down, taps, out): taps of length 0 = the default design; out holds ceil(len up / down)
 * outputs.  upfirdn(h, signal, up, down, out): out holds ((len - 1) up + ntaps - 1) / down + 1.  Arguments the library
 * refuses reach it unchanged (it fails before touching the output), so its message is what the caller sees.
 * [ROADMAP.md, "Filters and utilities"; include/pdsp_hip.h, "polyphase rate change"] */
static napi_value ResamplePoly(napi_env env, napi_callback_info info) {
  args a;
  args_read(&a, env, info, 5);
  const int64_t up = arg_i64(&a, 1), down = arg_i64(&a, 2);
  const f64_span x = arg_f64s(&a, 0), h = arg_f64s(&a, 3), y = arg_f64s(&a, 4);
  if (!a.ok) return NULL;
  if (ratio_ok(up, down) && x.n >= 1 && !holds(y, ((int64_t)x.n * up + down - 1) / down)) /* x.n < 2^53, up <= 8192 */
    return refuse(env, "pdsp_napi: resamplePoly output too small");
  return done(env, pdsp_resample_poly_host_f64(x.p, 1, (long long)x.n, up, down, h.n ? h.p : NULL, (long long)h.n,
                                               y.p));
}

static napi_value Upfirdn(napi_env env, napi_callback_info info) {
  args a;
  args_read(&a, env, info, 5);
  const int64_t up = arg_i64(&a, 2), down = arg_i64(&a, 3);
  const f64_span h = arg_f64s(&a, 0), x = arg_f64s(&a, 1), y = arg_f64s(&a, 4);
  if (!a.ok) return NULL;
  if (ratio_ok(up, down) && x.n >= 1 && h.n >= 1 && h.n <= RATIO_MAX &&
      !holds(y, (((int64_t)x.n - 1) * up + (int64_t)h.n - 1) / down + 1))
    return refuse(env, "pdsp_napi: upfirdn output too small");
  return done(env, pdsp_upfirdn_host_f64(h.p, (long long)h.n, x.p, 1, (long long)x.n, up, down, y.p));
}

/* resampleDesign(up, down, out) -> the number of taps; out of length 0 asks for the count alone */
static napi_value ResampleDesign(napi_env env, napi_callback_info info) {
  args a;
  napi_value res;
  args_read(&a, env, info, 3);
  const int64_t up = arg_i64(&a, 0), down = arg_i64(&a, 1);
  const f64_span h = arg_f64s(&a, 2);
  if (!a.ok) return NULL;
  long long n = 0;
  if (pdsp_resample_design_f64(up, down, NULL, &n) != PDSP_OK) return throw_pdsp(env);
  if (h.n) {
    if (!holds(h, n)) return refuse(env, "pdsp_napi: resampleDesign output too small");
    if (pdsp_resample_design_f64(up, down, h.p, &n) != PDSP_OK) return throw_pdsp(env);
  }
  NAPI_OK_OR_THROW(env, napi_create_int64(env, n, &res));
  return res;
}

/* ---- short-time transforms ------------------------------------------------------------------------------------ */

/* frames of `size` samples every `hop` in a signal of `len` >= size samples */
static int64_t frame_count(size_t len, int64_t size, int64_t hop) { return 1 + ((int64_t)len - size) / hop; }

/* stft(signal, fftSize, hopSize, windowType, real, imag): real / imag receive F x (fftSize/2 + 1) bins,
 * F = 1 + (len - fftSize) / hopSize.  Arguments the library refuses reach it unchanged (it fails before touching the
 * outputs), so its message is what the caller sees. */
static napi_value Stft(napi_env env, napi_callback_info info) {
  args a;
  args_read(&a, env, info, 6);
  const int64_t n = arg_i64(&a, 1), hop = arg_i64(&a, 2);
  const int win = arg_int(&a, 3, -1);
  const f64_span x = arg_f64s(&a, 0), re = arg_f64s(&a, 4), im = arg_f64s(&a, 5);
  if (!a.ok) return NULL;
  if (n >= PACKED_MIN && n <= PACKED_MAX && hop >= 1 && (int64_t)x.n >= n) {
    const int64_t need = extent(frame_count(x.n, n, hop), n / 2 + 1);
    if (!holds(re, need) || !holds(im, need)) return refuse(env, "pdsp_napi: stft output too small");
  }
  return done(env, pdsp_stft_host_f64(x.p, (long long)x.n, n, hop, win, re.p, im.p));
}

/* sdft(signal, size, bins, hop, windowType, real, imag): real / imag receive bins.length series of F values,
 * F = 1 + (len - size) / hop, of the sliding DFT of one signal (include/pdsp_hip.h, "sliding DFT").  Arguments the
 * library refuses reach it unchanged (it fails before touching the outputs), so its message is what the caller sees. */
static napi_value Sdft(napi_env env, napi_callback_info info) {
  args a;
  args_read(&a, env, info, 7);
  const int64_t n = arg_i64(&a, 1), hop = arg_i64(&a, 3);
  const int win = arg_int(&a, 4, -1);
  const f64_span x = arg_f64s(&a, 0), bins = arg_f64s(&a, 2), re = arg_f64s(&a, 5), im = arg_f64s(&a, 6);
  if (!a.ok) return NULL;
  if (n >= 2 && n <= PACKED_MAX && hop >= 1 && (int64_t)x.n >= n && bins.n >= 1 && bins.n <= SDFT_BINS_MAX) {
    const int64_t need = extent(frame_count(x.n, n, hop), (int64_t)bins.n);
    if (!holds(re, need) || !holds(im, need)) return refuse(env, "pdsp_napi: sdft output too small");
  }
  return done(env, pdsp_sdft_host_f64(x.p, 1, (long long)x.n, n, (long long)bins.n, bins.p, hop, win, re.p, im.p));
}

/* istft(real, imag, frames, fftSize, hopSize, windowType, out): out receives (frames - 1) hopSize + fftSize samples. */
static napi_value Istft(napi_env env, napi_callback_info info) {
  args a;
  args_read(&a, env, info, 7);
  const int64_t frames = arg_i64(&a, 2), n = arg_i64(&a, 3), hop = arg_i64(&a, 4);
  const int win = arg_int(&a, 5, -1);
  const f64_span re = arg_f64s(&a, 0), im = arg_f64s(&a, 1), y = arg_f64s(&a, 6);
  if (!a.ok) return NULL;
  if (n >= PACKED_MIN && n <= PACKED_MAX && hop >= 1 && frames >= 1) {
    /* an extent that overflows, or exceeds the library's 2^40 bound, goes to the library, which refuses it */
    const int64_t limit = (int64_t)1 << 40, need_in = extent(frames, n / 2 + 1), span = extent(frames - 1, hop);
    if (need_in <= limit && span <= limit - n && (!holds(re, need_in) || !holds(im, need_in) || !holds(y, span + n)))
      return refuse(env, "pdsp_napi: istft buffers too small");
  }
  return done(env, pdsp_istft_host_f64(re.p, im.p, frames, n, hop, win, y.p));
}

/* ---- the later row families ----------------------------------------------------------------------------------- */

/* dct(type, norm, x, y): y receives the dct of one signal of x.length values (type 2 / 3, norm a pdsp_dct_norm).  A
 * length the library refuses reaches it unchanged, so its message is what the caller sees. */
static napi_value Dct(napi_env env, napi_callback_info info) {
  args a;
  args_read(&a, env, info, 4);
  const int type = arg_int(&a, 0, 0); /* refused by the library as "type must be 2 or 3" */
  const int norm = arg_int(&a, 1, -1);
  const f64_span x = arg_f64s(&a, 2), y = arg_f64s(&a, 3);
  if (!a.ok) return NULL;
  if (y.n < x.n) return refuse(env, "pdsp_napi: dct output too small");
  return done(env, pdsp_dct_host_f64(x.p, 1, (long long)x.n, type, norm, y.p));
}

/* hilbert(mode, n, x, y): y receives n values (mode 0, analytic: 2n, interleaved) of one signal of x.length <= n
 * samples zero-padded to n (mode a pdsp_hilbert_out).  A size the library refuses reaches it unchanged (it fails
 * before touching y), so its message is what the caller sees. */
static napi_value Hilbert(napi_env env, napi_callback_info info) {
  args a;
  args_read(&a, env, info, 4);
  const int mode = arg_int(&a, 0, -1); /* refused by the library as an unknown output */
  const int64_t n = arg_i64(&a, 1);
  const f64_span x = arg_f64s(&a, 2), y = arg_f64s(&a, 3);
  if (!a.ok) return NULL;
  if (n >= PACKED_MIN && n <= PACKED_MAX && !holds(y, mode == PDSP_HILBERT_ANALYTIC ? 2 * n : n))
    return refuse(env, "pdsp_napi: hilbert output too small");
  return done(env, pdsp_hilbert_host_f64(x.p, 1, (long long)x.n, n, mode, y.p));
}

/* dft(inverse, re, im, outRe, outIm): the DFT (inverse != 0: the inverse DFT) of one row of re.length points, any
 * length 2 ... 4096; im null or undefined means a real row.  A length the library refuses reaches it unchanged (it
 * fails before touching the outputs), so its message is what the caller sees. */
static napi_value Dft(napi_env env, napi_callback_info info) {
  args a;
  args_read(&a, env, info, 5);
  const int64_t inverse = arg_i64(&a, 0);
  const f64_span re = arg_f64s(&a, 1), im = arg_f64s(&a, 2), ore = arg_f64s(&a, 3), oim = arg_f64s(&a, 4);
  if (!a.ok) return NULL;
  if (im.p && im.n != re.n) return refuse(env, "pdsp_napi: dft real and imag lengths differ");
  if (re.n >= 2 && re.n <= DFT_MAX && (ore.n < re.n || oim.n < re.n)) return refuse(env, "pdsp_napi: dft output too small");
  return done(env, pdsp_dft_host_f64(re.p, im.p, 1, (long long)re.n, inverse != 0, ore.p, oim.p));
}

/* czt(bins, step, start, radius, re, im, outRe, outIm): bins points of the chirp-z transform of one row of re.length
 * samples (include/pdsp_hip.h: step and start in turns); im null or undefined means a real row.  Sizes the library
 * refuses reach it unchanged (it fails before touching the outputs), so its message is what the caller sees. */
static napi_value Czt(napi_env env, napi_callback_info info) {
  args a;
  args_read(&a, env, info, 8);
  const int64_t bins = arg_i64(&a, 0);
  const double step = arg_f64(&a, 1), start = arg_f64(&a, 2), radius = arg_f64(&a, 3);
  const f64_span re = arg_f64s(&a, 4), im = arg_f64s(&a, 5), ore = arg_f64s(&a, 6), oim = arg_f64s(&a, 7);
  if (!a.ok) return NULL;
  if (im.p && im.n != re.n) return refuse(env, "pdsp_napi: czt real and imag lengths differ");
  if (re.n >= 1 && bins >= 1 && re.n <= RATIO_MAX && bins <= RATIO_MAX && (int64_t)re.n + bins - 1 <= RATIO_MAX &&
      (!holds(ore, bins) || !holds(oim, bins)))
    return refuse(env, "pdsp_napi: czt output too small");
  return done(env, pdsp_czt_host_f64(re.p, im.p, 1, (long long)re.n, bins, step, start, radius, ore.p, oim.p));
}

/* dwt(mode, name, taps, levels, x, y): mode 0 = wavedec, 1 = waverec of one row of x.length values into y, with the
 * built-in wavelet `name` (a string) or, name null, the caller's taps; mode 2 = the taps of `name` into y, returning
 * their number (y of length 0 asks for the number alone).  Arguments the library refuses reach it unchanged (it fails
 * before touching y), so its message is what the caller sees. */
static napi_value Dwt(napi_env env, napi_callback_info info) {
  args a;
  napi_value res;
  char buf[40];
  args_read(&a, env, info, 6);
  const int64_t mode = arg_i64(&a, 0);
  const int levels = arg_int(&a, 3, 0); /* refused by the library as "levels must be >= 1" */
  const char *name = arg_str(&a, 1, buf, sizeof(buf));
  const f64_span h = arg_f64s(&a, 2), x = arg_f64s(&a, 4), y = arg_f64s(&a, 5);
  if (!a.ok) return NULL;
  if (mode == 2) {
    long long n = 0;
    if (pdsp_wavelet_taps(name, NULL, &n) != PDSP_OK) return throw_pdsp(env);
    if (y.n) {
      if (!holds(y, n)) return refuse(env, "pdsp_napi: dwt output too small");
      if (pdsp_wavelet_taps(name, y.p, &n) != PDSP_OK) return throw_pdsp(env);
    }
    NAPI_OK_OR_THROW(env, napi_create_int64(env, n, &res));
    return res;
  }
  if (y.n < x.n) return refuse(env, "pdsp_napi: dwt output too small");
  const int rc = mode ? pdsp_dwt_inverse_host_f64(x.p, 1, (long long)x.n, name, h.p, (long long)h.n, levels, y.p)
                      : pdsp_dwt_forward_host_f64(x.p, 1, (long long)x.n, name, h.p, (long long)h.n, levels, y.p);
  return done(env, rc);
}

/* ntt(mode, a, b, n, y): mode 0 = the transform, 1 = its inverse of one row of a.length = n points into y (b null);
 * mode 2 = the first y.length values of the n-point cyclic product of the rows a and b.  Sizes the library refuses
 * reach it unchanged (it fails before touching y), so its message is what the caller sees. */
static napi_value Ntt(napi_env env, napi_callback_info info) {
  args a;
  args_read(&a, env, info, 5);
  const int64_t mode = arg_i64(&a, 0), n = arg_i64(&a, 3);
  const u64_span x = arg_u64s(&a, 1), b = arg_u64s(&a, 2), y = arg_u64s(&a, 4);
  if (!a.ok) return NULL;
  int rc;
  if (mode == 2) {
    rc = pdsp_ntt_conv_host_u64(x.p, (long long)x.n, b.p, (long long)b.n, 1, 1, n, y.p, (long long)y.n);
  } else {
    if ((int64_t)x.n != n) return refuse(env, "pdsp_napi: ntt input length differs from the size");
    if (n >= PACKED_MIN && n <= PACKED_MAX && (int64_t)y.n < n) return refuse(env, "pdsp_napi: ntt output too small");
    rc = pdsp_ntt_host_u64(x.p, 1, n, mode != 0, y.p);
  }
  return done(env, rc);
}

static napi_value Init(napi_env env, napi_value exports) {
  const struct {
    const char *name;
    napi_callback fn;
  } fns[] = {
      {"planCreate", PlanCreate}, {"transform", Transform},   {"windowMake", WindowMake},
      {"transformBatch", TransformBatch}, {"transformRows", TransformRows},
      {"applyWindow", ApplyWindow}, {"magnitude", Magnitude}, {"phase", Phase},
      {"spectrum", Spectrum},     {"binFrequencies", BinFrequencies}, {"fftShift", FftShift},
      {"spectrumBatch", SpectrumBatch}, {"spectrumRows", SpectrumRows},
      {"nextPow2", NextPow2},     {"deviceCount", DeviceCount},
      {"firFilter", FirFilter},   {"resamplePoly", ResamplePoly}, {"upfirdn", Upfirdn},
      {"resampleDesign", ResampleDesign},   {"stft", Stft},               {"istft", Istft},
      {"dct", Dct},                 {"hilbert", Hilbert},         {"dft", Dft},
      {"dwt", Dwt},                 {"czt", Czt},                 {"ntt", Ntt},
      {"sdft", Sdft},
  };
  for (size_t i = 0; i < sizeof(fns) / sizeof(fns[0]); ++i) {
    napi_value f;
    if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok) return NULL;
    if (napi_set_named_property(env, exports, fns[i].name, f) != napi_ok) return NULL;
  }
  napi_value ver;
  if (napi_create_int32(env, pdsp_version(), &ver) == napi_ok) napi_set_named_property(env, exports, "version", ver);
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)

// pdsp_capi.hip -- the core of the host side of the C ABI (include/pdsp_hip.h): error state, the scratch pools and
// live counters, the development switches, the plan object with its table builders and the plan cache, windows and
// host index math, the plane layout, and the device-pointer transforms, spectra and element-wise entry points with
// their pdsp_dev_* path queries.  It also defines, once, the helpers pdsp_host.h declares for the other host units:
//   pdsp_capi_host.hip      the f64 drop-in (chunked host calls of transforms and spectra)
//   pdsp_capi_<family>.hip  one unit per family: fir, stft, dct, hilbert, resample, chirp, dwt, ntt, sdft, fft2d
//
// Host side only: no kernel is instantiated in any pdsp_capi*.hip (the dispatchers they call -- run_complex,
// spectrum_impl, ... -- are declared in pdsp_internal.h and live in the pdsp_kernels_*.hip units).
//
// Product path only: nothing here touches oracle/, and there is no CPU fallback --
// without a HIP device every compute entry point fails with PDSP_ERR_DEVICE.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <climits>
#include <cstring>
#include <atomic>
#include <initializer_list>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "pdsp_host.h"

namespace pdsp_host {

thread_local std::string g_err;
// development switches (tools / tests): 0 routes N = 16384 spectra to spectrum_packed_kernel<13>,
// and 32 <= N <= 256 transforms to the direct kernel instead of fft_staged_kernel
int g_split16k = 1;
int g_fused_window = 1;  // pdsp_set_fused_window: plan-owned cosine-sum windows evaluated in the kernel
int g_twopass = 1;       // pdsp_set_twopass: 2^15 <= N <= 2^18 f32 transforms in two passes (balanced factors)
int g_split8k_f32 = 0;  // f32 N = 8192 rows on fft_split2_kernel too (A/B: pdsp_set_split16k bit 1)
int g_staged_small = 1;
int g_real_packed = 1;  // pdsp_set_real_packed: Radix2Fft.forward rows of 512 <= N <= 16384 on fft_real_kernel

int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

constexpr int kMaxPoolDevices = 64;
hipMemPool_t g_scratch_pool[kMaxPoolDevices] = {};
std::mutex g_scratch_pool_mu;
hipMemPool_t scratch_pool() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxPoolDevices) return nullptr;
  std::lock_guard<std::mutex> lk(g_scratch_pool_mu);
  if (!g_scratch_pool[dev]) {
    hipMemPoolProps props = {};
    props.allocType = hipMemAllocationTypePinned;
    props.location.type = hipMemLocationTypeDevice;
    props.location.id = dev;
    hipMemPool_t pool = nullptr;
    if (hipMemPoolCreate(&pool, &props) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    uint64_t keep = ~0ULL;
    (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    g_scratch_pool[dev] = pool;
  }
  return g_scratch_pool[dev];
}
std::atomic<unsigned long long> g_scratch_drawn{0};
LiveCounters g_live;

void trim_scratch_pools() {
  std::lock_guard<std::mutex> lk(g_scratch_pool_mu);
  for (hipMemPool_t pool : g_scratch_pool)
    if (pool) (void)hipMemPoolTrimTo(pool, 0);
  g_scratch_drawn = 0;
}

}  // namespace pdsp_host

using namespace pdsp_host;

namespace {

// The plan's staging buffers go back (g_live counts the buffers, not their bytes).  Caller holds plan->mu, or is the
// last user of the plan.
void free_host_stage(pdsp_plan *plan) {
  if (!plan->h_stage) return;
  (void)hipHostFree(plan->h_stage);
  --g_live.host_stage;
  plan->h_stage = nullptr;
  plan->h_bytes = 0;
}
void free_dev_stage(pdsp_plan *plan) {
  if (!plan->d_stage) return;
  (void)hipFree(plan->d_stage);
  --g_live.dev_stage;
  plan->d_stage = nullptr;
  plan->d_bytes = 0;
}

// Appends `count` pairs (cos, sin) of angle(k), k = 0 ... count - 1, evaluated in f64 and rounded once (P: a T2, or
// float2 for the flat float pair tables).  Every caller spells its angle out as the kernels' derivations do:
// (-2 pi k) / N and f * 4096 * i do not round like a normalised form of the same angle, and the tables are pinned bit
// for bit.
template <typename P, class Angle>
void add_cos_sin(std::vector<P> &w, size_t count, Angle angle) {
  w.reserve(w.size() + count);
  for (size_t k = 0; k < count; ++k) {
    const double a = angle(k);
    P v;
    v.x = (decltype(v.x))std::cos(a);
    v.y = (decltype(v.y))std::sin(a);
    w.push_back(v);
  }
}

// `tw` of the N2-point rows, and the split kernels' W_N2^k for rows of 16384 and 8192 points
template <typename T>
hipError_t upload_transform_tables(Tables<T> &t) {
  using T2 = typename pdsp::vec2<T>::type;
  if (hipError_t e = upload_table(t, build_twiddles<T2>(t.log2n2), &t.tw)) return e;
  std::vector<T2> w;
  if (t.log2n2 == 14) {  // fft_split4_kernel: W_16384^k, k < 768
    add_cos_sin(w, 768, [](size_t k) { return (-2.0 * M_PI * (double)k) / 16384.0; });
    return upload_table(t, w, &t.tws4);
  }
  if (t.log2n2 == 13) {  // fft_split2_kernel: W_8192^k, k < 256
    add_cos_sin(w, 256, [](size_t k) { return (-2.0 * M_PI * (double)k) / 8192.0; });
    return upload_table(t, w, &t.tws2);
  }
  return hipSuccess;
}

// Radix tables of the balanced factors of a 2^lg-point transform in tile passes: two factors up to 2^18 (2^18 =
// 512 * 512), three above; ascending, so that the widest tiles serve the passes with two strided streams
template <typename T>
hipError_t upload_factor_tables(Tables<T> &t, int lg, int *np, int *l, typename pdsp::vec2<T>::type **tw) {
  if (lg <= 18) {
    *np = 2;
    l[0] = lg / 2, l[1] = lg - l[0];
  } else {
    *np = 3;
    three_factors(lg, l);
  }
  for (int i = 0; i < *np; ++i)
    if (hipError_t e = upload_table(t, build_twiddles<typename pdsp::vec2<T>::type>(l[i]), &tw[i])) return e;
  return hipSuccess;
}

// The multi-pass paths (N beyond the single-pass limit): W_N^m = twa[m >> 9] * twb[m & 511], the tile passes of the
// f32 transform and of the packed-real spectrum's N/2-point transform, and the general four-step path's row table
template <typename T>
hipError_t upload_multipass_tables(Tables<T> &t, int log2n, long long size) {
  using T2 = typename pdsp::vec2<T>::type;
  std::vector<T2> a, b;
  add_cos_sin(a, (size_t)(size >> 9), [&](size_t i) { return (-2.0 * M_PI * (double)(i << 9)) / (double)size; });
  add_cos_sin(b, 512, [&](size_t i) { return (-2.0 * M_PI * (double)i) / (double)size; });
  if (hipError_t e = upload_table(t, a, &t.twa)) return e;
  if (hipError_t e = upload_table(t, b, &t.twb)) return e;
  if (sizeof(T) == 4 && log2n >= 15 && log2n <= 27) {  // tile passes (tile_pass_kernel's header)
    // tile_cols512_kernel / tile_rows512_kernel run a 512-point factor as two 256-point halves
    if (hipError_t e = upload_table(t, build_twiddles<T2>(8), &t.tw8)) return e;
    if (hipError_t e = upload_factor_tables(t, log2n, &t.tp_np, t.tp_l, t.tp_tw)) return e;
    // the N/2-point transform of the packed-real spectrum path (at 2^18 = 512 * 512 the packed first pass on
    // 16-column tiles still reads 128-byte segments, eight samples per lane)
    if (hipError_t e = upload_factor_tables(t, log2n - 1, &t.hp_np, t.hp_l, t.hp_tw)) return e;
    // fused createWindow on the packed first pass (tile_pass_kernel IN = 5 / 6; fourier.ts:14-52:
    // f = 2 pi / (size - 1)): cs(f n) by angle addition, tables built in f64.  The kernels index the parts by their
    // sizes (TileGeom::wa ...): wa | wb | wstep | we | wq (fft_split4_kernel's packed loader, N = 2^15)
    const double f = 2.0 * M_PI / (double)(size - 1);
    const long long in_stride = (size / 2) >> t.hp_l[0];  // points between the rows of a column
    const int spi = 1024 / tile_width(t.hp_l[0]);         // tile_pass_kernel's SPI
    t.hp_win_a = (size_t)((size / 8 + 511) / 512);
    std::vector<float2> w;
    add_cos_sin(w, t.hp_win_a, [&](size_t i) { return f * 4096.0 * (double)i; });
    add_cos_sin(w, 512, [&](size_t j) { return f * 8.0 * (double)j; });
    add_cos_sin(w, 8, [&](size_t ic) { return f * 2.0 * (double)in_stride * (double)spi * (double)ic; });
    add_cos_sin(w, 8, [&](size_t ee) { return f * (double)ee; });
    add_cos_sin(w, 16, [&](size_t q) { return f * 2048.0 * (double)q; });
    if (hipError_t e = upload_table(t, w, &t.hp_win)) return e;
  }
  if (t.log2n1 > pdsp::kMaxLog2N1) return upload_table(t, build_twiddles<T2>(t.log2n1), &t.tw1);
  return hipSuccess;
}

// The packed-real paths (64 <= N, N/2 single-pass): radix table of the N/2-point transform, the split twiddles
// W_N^k, 0 <= k <= N/4, and up to N = 16384 the DCT twiddles W_4N^k, 0 <= k <= N/2
template <typename T>
hipError_t upload_packed_tables(Tables<T> &t, int log2n, long long size) {
  using T2 = typename pdsp::vec2<T>::type;
  if (hipError_t e = upload_table(t, build_twiddles<T2>(log2n - 1), &t.tw_half)) return e;
  std::vector<T2> twr, tw4;
  add_cos_sin(twr, (size_t)(size / 4 + 1), [&](size_t k) { return (-2.0 * M_PI * (double)k) / (double)size; });
  if (hipError_t e = upload_table(t, twr, &t.twr)) return e;
  if (log2n > 14) return hipSuccess;
  add_cos_sin(tw4, (size_t)(size / 2 + 1), [&](size_t k) { return (-M_PI * (double)k) / (2.0 * (double)size); });
  return upload_table(t, tw4, &t.tw4n);
}

// Fused createWindow of the f32 single-pass spectrum kernels (fourier.ts:14-52: f = 2 pi / (size - 1)), angle-addition
// tables built in f64: a frame on `tp` threads takes sample n = (2 tid + e) + 2 tp q, so wf_base holds cs(f (2 tid + e))
// and wf_step cs(f 2 tp q), q < 16.  N = 16384 (spectrum_dif16k_kernel, 256 threads) has 16 more steps, at + 8192.
hipError_t upload_fused_window_tables(Tables<float> &t, int tp, long long size) {
  const double f = 2.0 * M_PI / (double)(size - 1);
  std::vector<float2> base, step;
  add_cos_sin(base, 2 * (size_t)tp, [&](size_t n) { return f * (double)n; });
  add_cos_sin(step, 16, [&](size_t q) { return f * 2.0 * tp * (double)q; });
  if (size == 16384) add_cos_sin(step, 16, [&](size_t q) { return f * (double)(2 * tp * (long long)q + 8192); });
  if (hipError_t e = upload_table(t, base, &t.wf_base)) return e;
  return upload_table(t, step, &t.wf_step);
}

// full: the N-point complex transform exists in this precision; half: so do the packed-real paths (pdsp_plan_create)
template <typename T>
hipError_t upload_tables(Tables<T> &t, int log2n, long long size, bool full, bool half) {
  using T2 = typename pdsp::vec2<T>::type;
  if (full) {
    t.log2n2 = log2n > max_log2n<T>() ? max_log2n<T>() : log2n;
    t.log2n1 = log2n - t.log2n2;
    if (hipError_t e = upload_transform_tables(t)) return e;
    if (t.log2n1 > 0)
      if (hipError_t e = upload_multipass_tables(t, log2n, size)) return e;
  }
  // radix table of the 4096-point sub-transforms: the split kernels on rows of 16384 and 8192 points, and the
  // packed-real kernels at N = 16384
  if ((full && (t.log2n2 == 14 || t.log2n2 == 13)) || (half && log2n == 14))
    if (hipError_t e = upload_table(t, build_twiddles<T2>(12), &t.tw12)) return e;
  if (!half) return hipSuccess;
  if (hipError_t e = upload_packed_tables(t, log2n, size)) return e;
  if constexpr (sizeof(T) == 4) {
    if (log2n >= 10 && log2n <= 13) return upload_fused_window_tables(t, (int)(size / 32), size);  // spectrum_packed_kernel
    if (log2n == 14) return upload_fused_window_tables(t, 256, size);
  }
  return hipSuccess;
}

template <typename T>
int apply_window_checked(long long batch, long long n, const T *in, const T *window, T *out, hipStream_t s) {
  if (batch < 0 || n < 0) return fail(PDSP_ERR_BAD_ARG, "negative size");
  long long total = 0;
  if (!mad_ok(batch, n, 0, &total) || total > (LLONG_MAX / 8))
    return fail(PDSP_ERR_BAD_ARG, "batch %lld x n overflows", batch);
  if (total == 0) return PDSP_OK;
  if (!in || !window || !out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const size_t bytes = (size_t)total * sizeof(T);
  if (elementwise_clash(out, in, bytes) || host_ranges_overlap(out, bytes, window, (size_t)n * sizeof(T)))
    return fail(PDSP_ERR_BAD_ARG, "output overlaps input");
  return apply_window_dev<T>(batch, n, in, window, out, s);
}

template <typename T, bool PHASE>
int polar_checked(long long count, const T *re, const T *im, T *out, hipStream_t s) {
  if (count < 0) return fail(PDSP_ERR_BAD_ARG, "negative size");
  if (count > (LLONG_MAX / 8)) return fail(PDSP_ERR_BAD_ARG, "count %lld overflows", count);
  if (count == 0) return PDSP_OK;
  if (!re || !im || !out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const size_t bytes = (size_t)count * sizeof(T);
  if (elementwise_clash(out, re, bytes) || elementwise_clash(out, im, bytes))
    return fail(PDSP_ERR_BAD_ARG, "output overlaps input");
  return polar_dev<T, PHASE>(count, re, im, out, s);
}

}  // namespace

// ---- what pdsp_host.h declares: defined once, here ------------------------------------------------------------

namespace pdsp_host {

// The plan's own stream, created on first use.  Caller holds plan->mu.
int ensure_plan_stream(pdsp_plan *plan) {
  if (!plan->stream) {
    PDSP_HIP_TRY(hipStreamCreateWithFlags(&plan->stream, hipStreamNonBlocking));
    ++g_live.streams;
  }
  return PDSP_OK;
}

int ensure_stage(pdsp_plan *plan, size_t bytes) {
  if (int rc = ensure_plan_stream(plan)) return rc;
  if (plan->h_bytes < bytes) {
    free_host_stage(plan);
    PDSP_HIP_TRY(hipHostMalloc(&plan->h_stage, bytes, hipHostMallocDefault));
    ++g_live.host_stage;
    plan->h_bytes = bytes;
  }
  if (plan->d_bytes < bytes) {
    free_dev_stage(plan);
    PDSP_HIP_TRY(hipMalloc(&plan->d_stage, bytes));
    ++g_live.dev_stage;
    plan->d_bytes = bytes;
  }
  return PDSP_OK;
}

// Plans for the one-shot host entry points, keyed by (size, device): the idea of
// FourierLive's `Map<size, FFT>` and `Map<"type:size", window>` caches
// (src/effect/index.ts:30-48).  The reference's spectrum() rebuilds both on every call
// (spectrum.ts:114-116) -- its dominant one-shot cost; here a repeat call costs no table
// build, no hipMalloc and no upload.  Leaked on purpose at exit (the HIP runtime may
// already be gone when static destructors run); pdsp_plan_cache_clear() frees it.
// Bounded: at most kMaxCachedPlans entries, least recently used evicted first (an entry a call is
// still running on is pinned and never evicted), so a long-running host that calls spectrum() with
// ever-changing lengths keeps a bounded set of tables, streams and staging buffers.
constexpr size_t kMaxCachedPlans = 16;
PlanCache &plan_cache() {
  static PlanCache *c = new PlanCache();
  return *c;
}

int cached_plan(long long n, CachedPlan *out) {
  int dev = 0;
  PDSP_HIP_TRY(hipGetDevice(&dev));
  PlanCache &c = plan_cache();
  std::lock_guard<std::mutex> lk(c.mu);
  const std::pair<long long, int> key{n, dev};
  auto it = c.plans.find(key);
  if (it == c.plans.end()) {
    // make room first: drop least-recently-used entries nobody is running on
    while (c.plans.size() >= kMaxCachedPlans) {
      auto victim = c.plans.end();
      for (auto jt = c.plans.begin(); jt != c.plans.end(); ++jt)
        if (jt->second.pins == 0 && (victim == c.plans.end() || jt->second.last_use < victim->second.last_use)) victim = jt;
      if (victim == c.plans.end()) break;  // every entry is in use: grow past the bound rather than block
      pdsp_plan_destroy(victim->second.plan);
      c.plans.erase(victim);
      ++g_live.evictions;
    }
    pdsp_plan *p = nullptr;
    if (int rc = pdsp_plan_create(n, dev, &p)) return rc;
    it = c.plans.emplace(key, PlanCache::Entry{p, 0, 0}).first;
  }
  it->second.last_use = ++c.tick;
  ++it->second.pins;
  out->plan = it->second.plan;
  out->key = key;
  return PDSP_OK;
}

// Staging above this size is handed back after the call that needed it (a one-off long frame or
// large batch must not pin host memory and HBM for the life of the plan); smaller staging stays, so
// repeat calls of ordinary sizes still cost no allocation.  Caller holds plan->mu.
constexpr size_t kStageKeepBytes = (size_t)64 << 20;
void trim_stage(pdsp_plan *plan) {
  if (plan->h_bytes > kStageKeepBytes) free_host_stage(plan);
  if (plan->d_bytes > kStageKeepBytes) free_dev_stage(plan);
}

// A table still to be uploaded on a caller's stream that is being captured: upload_table's hipMalloc and hipMemcpy are
// synchronous, which a capture forbids, and either would invalidate the capture it ran into.  Asked only where the
// table is missing and the stream is not the null stream; refused before anything is allocated or copied, so the capture
// stays valid and the handle usable ("Streams and graphs").
int refuse_upload_in_capture(hipStream_t s, const char *what) {
  if (!s) return PDSP_OK;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  PDSP_HIP_TRY(hipStreamIsCapturing(s, &st));
  if (st == hipStreamCaptureStatusNone) return PDSP_OK;
  return fail(PDSP_ERR_BAD_ARG,
              "stream is capturing: the %s is uploaded on the handle's first call in a precision, which no capture "
              "allows; make one call on this handle outside the capture first",
              what);
}

int require_device() {
  int count = 0;
  const hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    (void)hipGetLastError();
    return fail(PDSP_ERR_DEVICE, "no HIP device available (the pdsp engine has no CPU fallback) [hipGetDeviceCount: %s, %d]",
                hipGetErrorString(e), count);
  }
  return PDSP_OK;
}

// Which device a request means and whether it is visible: the current device for a negative request.  (Whether there is
// a device at all is require_device()'s question, asked where each caller has always asked it.)
int resolve_device(int *device) {
  int count = 0;
  PDSP_HIP_TRY(hipGetDeviceCount(&count));
  if (*device < 0) PDSP_HIP_TRY(hipGetDevice(device));
  if (*device >= count) return fail(PDSP_ERR_BAD_ARG, "device %d out of range (%d visible)", *device, count);
  return PDSP_OK;
}

// The extents of a call's operands, each of which must be computable and stay within LLONG_MAX / 8 elements, so that
// its byte size in either precision is computable too.  A call of no rows has operands of no extent.
int row_extents(long long batch, std::initializer_list<RowExtent> operands) {
  for (const RowExtent &r : operands) {
    long long rows = 0;
    *r.count = 0;
    if (batch > 0 && (!mad_ok(batch, r.per_batch, -1, &rows) || !mad_ok(rows, r.stride, r.len, r.count) ||
                      *r.count > (LLONG_MAX / 8)))
      return fail(PDSP_ERR_BAD_ARG, "batch %lld x stride overflows", batch);
  }
  return PDSP_OK;
}

// The packed-real kernels (FIR filtering, the short-time pair, the DCT) run on the N/2-point tables, N = 64 ... 16384
// in both precisions; the DCT also on W_4N^k.  `what` names the feature in the error text.
int packed_size_error(const char *what, long long n) {
  return fail(PDSP_ERR_UNSUPPORTED_SIZE, "%s needs a plan of 64 <= N <= 16384, got %lld", what, n);
}

// The same gate for the bare size of a host form, behind the power-of-two check of the plan it will ask for.
int check_packed_size(long long n, const char *what) {
  if (!pdsp_is_pow2(n)) return fail(PDSP_ERR_SIZE_NOT_POW2, "FFT size must be power of two, got %lld", n);
  if (n < 64 || n > 16384) return packed_size_error(what, n);
  return PDSP_OK;
}

}  // namespace pdsp_host

extern "C" {

int pdsp_version(void) { return 100; }

const char *pdsp_last_error(void) { return g_err.c_str(); }

int pdsp_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return count;
}

int pdsp_max_size(int scalar_bytes) {  // incl. the four-step paths
  if (scalar_bytes == 4) return 1 << pdsp::kMaxLog2Big_f32;
  if (scalar_bytes == 8) return 1 << pdsp::kMaxLog2Big_f64;
  return 0;
}

// the development switches: each setter returns the previous value
int pdsp_set_split16k(int enabled) {
  g_split8k_f32 = (enabled & 2) ? 1 : 0;
  return std::exchange(g_split16k, enabled ? 1 : 0);
}
// bit 0: tile passes; bit 1: their first form; bit 2 (or any value but 1): no fft_paired_kernel
int pdsp_set_twopass(int enabled) { return std::exchange(g_twopass, enabled & 7); }
int pdsp_set_fused_window(int enabled) { return std::exchange(g_fused_window, enabled ? 1 : 0); }
int pdsp_set_staged_small(int enabled) { return std::exchange(g_staged_small, enabled ? 1 : 0); }
int pdsp_set_real_packed(int enabled) { return std::exchange(g_real_packed, enabled ? 1 : 0); }

#define PDSP_DEFINE_PLAN_WINDOW(SUFFIX, T)                                                                  \
  int pdsp_plan_window_##SUFFIX(pdsp_plan *plan, int type, const T **window_out) {                          \
    if (!plan || !window_out) return fail(PDSP_ERR_BAD_ARG, "null plan or output");                        \
    *window_out = nullptr;                                                                                 \
    if (type < PDSP_WIN_RECT || type > PDSP_WIN_BLACKMAN)                                                  \
      return fail(PDSP_ERR_WINDOW_TYPE, "Unsupported window type: %d", type);                              \
    std::lock_guard<std::mutex> lk(plan->mu);                                                              \
    DeviceGuard g(plan->device);                                                                           \
    PDSP_HIP_TRY(g.err);                                                                                   \
    return plan_window<T>(plan, type, window_out);                                                         \
  }
PDSP_DEFINE_PLAN_WINDOW(f32, float)
PDSP_DEFINE_PLAN_WINDOW(f64, double)
#undef PDSP_DEFINE_PLAN_WINDOW

/* ---- host index math ---------------------------------------------------- */

int pdsp_is_pow2(long long n) { return n > 0 && (n & (n - 1)) == 0; }

long long pdsp_next_pow2(long long n) {
  if (n <= 1) return 1;
  long long p = 1;
  while (p < n && p < (1LL << 62)) p <<= 1;
  return p;
}

int pdsp_window_make(int type, long long size, double *out) {
  if (size <= 0) return fail(PDSP_ERR_WINDOW_SIZE, "Window size must be positive, got %lld", size);
  if (!out) return fail(PDSP_ERR_BAD_ARG, "out is null");
  if (size == 1) {  // fourier.ts:18-20 returns [1] before looking at the type
    out[0] = 1.0;
    return PDSP_OK;
  }
  if (type < PDSP_WIN_RECT || type > PDSP_WIN_BLACKMAN)
    return fail(PDSP_ERR_WINDOW_TYPE, "Unsupported window type: %d", type);
  const double denom = (double)(size - 1);
  for (long long i = 0; i < size; ++i) {
    const double f = (2.0 * M_PI * (double)i) / denom;
    double v = 1.0;
    if (type == PDSP_WIN_HANN) v = 0.5 * (1.0 - std::cos(f));
    else if (type == PDSP_WIN_HAMMING) v = 0.54 - 0.46 * std::cos(f);
    else if (type == PDSP_WIN_BLACKMAN) v = 0.42 - 0.5 * std::cos(f) + 0.08 * std::cos(2.0 * f);
    out[i] = v;
  }
  return PDSP_OK;
}

int pdsp_bin_frequencies(long long size, double sample_rate, int sides, double *out, long long *bins_out) {
  if (size <= 0) return fail(PDSP_ERR_FFT_SIZE, "FFT size must be positive, got %lld", size);
  if (sample_rate <= 0) return fail(PDSP_ERR_SAMPLE_RATE, "Sample rate must be positive, got %.17g", sample_rate);
  const long long bins = sides == PDSP_SIDES_ONE ? size / 2 + 1 : size;
  if (bins_out) *bins_out = bins;
  if (out) {
    const double scale = sample_rate / (double)size;
    for (long long i = 0; i < bins; ++i) out[i] = (double)i * scale;
  }
  return PDSP_OK;
}

int pdsp_fft_shift_f64(const double *in, long long n, double *out) {
  if (n < 0 || (n > 0 && (!in || !out))) return fail(PDSP_ERR_BAD_ARG, "bad fftShift arguments");
  const long long mid = n / 2;
  for (long long i = 0; i < n; ++i) out[i] = in[(i + mid) % n];
  return PDSP_OK;
}

long long pdsp_find_peak_f64(const double *amp, long long bins) {
  if (!amp || bins <= 0) return 0;
  long long max_i = 0, nondc_i = 0;
  double max_v = amp[0], nondc_v = 0.0;
  bool has_nondc = false;
  for (long long i = 1; i < bins; ++i) {
    const double v = amp[i];
    if (v > nondc_v) {
      nondc_v = v;
      nondc_i = i;
    }
    if (v > 0) has_nondc = true;
    if (v > max_v) {
      max_v = v;
      max_i = i;
    }
  }
  return has_nondc ? nondc_i : max_i;
}

/* ---- plan ----------------------------------------------------------------- */

int pdsp_plan_create(long long size, int device, pdsp_plan **plan_out) {
  if (!plan_out) return fail(PDSP_ERR_BAD_ARG, "plan_out is null");
  *plan_out = nullptr;
  if (!pdsp_is_pow2(size)) return fail(PDSP_ERR_SIZE_NOT_POW2, "FFT size must be power of two, got %lld", size);
  const int log2n = ilog2ll(size);
  if (log2n > pdsp::kMaxLog2Big_f32)
    return fail(PDSP_ERR_UNSUPPORTED_SIZE, "FFT size %lld exceeds the supported maximum %d", size,
                1 << pdsp::kMaxLog2Big_f32);
  if (int rc = require_device()) return rc;
  if (int rc = resolve_device(&device)) return rc;
  DeviceGuard g(device);
  PDSP_HIP_TRY(g.err);
  pdsp_plan *p = new (std::nothrow) pdsp_plan();
  if (!p) return fail(PDSP_ERR_BAD_ARG, "out of host memory");
  p->n = size;
  p->log2n = log2n;
  p->device = device;
  // f32: single-pass up to 2^14, four-step with fused columns (N1 <= 16) up to 2^18, general
  // four-step (N1 x 2^14) up to 2^28; the packed-real spectrum tables exist for the single-pass sizes
  hipError_t e = upload_tables<float>(p->t32, log2n, size, true, log2n >= 6 && log2n <= pdsp::kMaxLog2N_f32);
  // f64: the complex transform single-pass up to 2^13 and four-step up to 2^26; the packed-real
  // spectrum (an N/2-point transform) up to N = 2^14
  if (e == hipSuccess)
    e = upload_tables<double>(p->t64, log2n, size, log2n <= pdsp::kMaxLog2Big_f64,
                              log2n >= 6 && log2n - 1 <= pdsp::kMaxLog2N_f64);
  if (e != hipSuccess) {
    p->t32.release();
    p->t64.release();
    delete p;
    return fail(PDSP_ERR_DEVICE, "HIP error %d (%s) while uploading the twiddle tables", (int)e, hipGetErrorString(e));
  }
  *plan_out = p;
  return PDSP_OK;
}

int pdsp_plan_cache_clear(void) {
  PlanCache &c = plan_cache();
  std::lock_guard<std::mutex> lk(c.mu);
  // entries a call is still running on stay (their pin is released by that call)
  for (auto it = c.plans.begin(); it != c.plans.end();) {
    if (it->second.pins == 0) {
      pdsp_plan_destroy(it->second.plan);
      it = c.plans.erase(it);
    } else {
      ++it;
    }
  }
  trim_scratch_pools();  // the multi-pass paths' scratch planes (StreamScratch) go back to the device
  return PDSP_OK;
}

int pdsp_dev_live_resources(long long info[PDSP_DEV_LIVE_INFO]) {
  if (!info) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  long long cached = 0, pinned = 0;
  {
    PlanCache &c = plan_cache();
    std::lock_guard<std::mutex> lk(c.mu);
    cached = (long long)c.plans.size();
    for (const auto &kv : c.plans) pinned += kv.second.pins > 0;
  }
  const long long v[PDSP_DEV_LIVE_INFO] = {cached, pinned, g_live.evictions.load(), g_live.tables.load(),
                                           g_live.table_bytes.load(), g_live.host_stage.load(), g_live.dev_stage.load(),
                                           g_live.streams.load()};
  std::memcpy(info, v, sizeof(v));
  return PDSP_OK;
}

int pdsp_plan_destroy(pdsp_plan *plan) {
  if (!plan) return PDSP_OK;
  {
    DeviceGuard g(plan->device);
    if (plan->stream) {
      (void)hipStreamSynchronize(plan->stream);
      (void)hipStreamDestroy(plan->stream);
      --g_live.streams;
    }
    for (hipStream_t st : plan->slot_streams) {
      (void)hipStreamSynchronize(st);
      (void)hipStreamDestroy(st);
      --g_live.streams;
    }
    // a plan of a multi-pass size that drew scratch planes: the freed planes go back to the device with it
    const bool multipass = plan->t32.log2n1 > 0 || plan->t64.log2n1 > 0;
    plan->t32.release();
    plan->t64.release();
    free_dev_stage(plan);
    free_host_stage(plan);
    if (multipass && g_scratch_drawn.load() > 0) {
      (void)hipDeviceSynchronize();  // stream-ordered frees complete before the pool can let go of them
      trim_scratch_pools();
    }
  }
  delete plan;
  return PDSP_OK;
}

long long pdsp_plan_size(const pdsp_plan *plan) { return plan ? plan->n : 0; }
int pdsp_plan_device(const pdsp_plan *plan) { return plan ? plan->device : -1; }

/* ---- plane layout ------------------------------------------------------------ */

struct pdsp_arena {
  int device = -1;
  void *parts[4] = {nullptr, nullptr, nullptr, nullptr};  // one entry (the arena) or up to four plain allocations
};

int pdsp_planes_alloc(const pdsp_plan *plan, long long batch, int scalar_bytes, int real_input, void **re_in,
                      void **im_in, void **re_out, void **im_out, pdsp_arena **arena, unsigned long long *arena_bytes) {
  if (!plan) return fail(PDSP_ERR_BAD_ARG, "plan is null");
  if (!re_in || !im_in || !re_out || !im_out || !arena) return fail(PDSP_ERR_BAD_ARG, "null output");
  if (batch <= 0) return fail(PDSP_ERR_BAD_ARG, "batch must be > 0, got %lld", batch);
  if (scalar_bytes != 4 && scalar_bytes != 8) return fail(PDSP_ERR_BAD_ARG, "scalar_bytes must be 4 or 8, got %d", scalar_bytes);
  *re_in = *im_in = *re_out = *im_out = nullptr;
  *arena = nullptr;
  if (arena_bytes) *arena_bytes = 0;
  // a plane is batch contiguous rows: a batch no launch could take, or a size that does not compute, allocates nothing
  long long count = 0;
  if (int rc = check_plan_batch(plan, batch)) return rc;
  if (int rc = row_extents(batch, {{plan->n, plan->n, &count}})) return rc;
  DeviceGuard g(plan->device);
  PDSP_HIP_TRY(g.err);
  const size_t gib = (size_t)1 << 30;
  const size_t plane = (size_t)count * (size_t)scalar_bytes;
  pdsp_arena *a = new (std::nothrow) pdsp_arena();
  if (!a) return fail(PDSP_ERR_BAD_ARG, "out of host memory");
  a->device = plan->device;
  if (plane >= ((size_t)256 << 20) && plane <= 8 * gib) {  // smaller planes have nothing to gain: plain allocations
    size_t free_b = 0, total_b = 0;
    const size_t need = 80 * gib + plane;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b >= need + 4 * gib) {
      void *base = nullptr;
      if (hipMalloc(&base, need) == hipSuccess) {
        a->parts[0] = base;
        char *b = (char *)base;
        *re_in = b;
        *im_in = real_input ? nullptr : b + ((plane + 255) & ~(size_t)255);
        *re_out = b + 40 * gib;
        *im_out = b + 80 * gib;
        *arena = a;
        if (arena_bytes) *arena_bytes = (unsigned long long)need;
        return PDSP_OK;
      }
      (void)hipGetLastError();
    }
  }
  // no room for the layout: four plain allocations
  void **outs[4] = {re_in, im_in, re_out, im_out};
  for (int i = 0; i < 4; ++i) {
    if (i == 1 && real_input) continue;
    const hipError_t e = hipMalloc(&a->parts[i], plane);
    if (e != hipSuccess) {
      for (void *p : a->parts)
        if (p) (void)hipFree(p);
      delete a;
      *re_in = *im_in = *re_out = *im_out = nullptr;
      return fail(PDSP_ERR_DEVICE, "HIP error %d (%s) at hipMalloc of a plane of %zu bytes", (int)e, hipGetErrorString(e), plane);
    }
    *outs[i] = a->parts[i];
  }
  *arena = a;
  return PDSP_OK;
}

int pdsp_planes_free(pdsp_arena *arena) {
  if (!arena) return PDSP_OK;
  DeviceGuard g(arena->device);
  for (void *p : arena->parts)
    if (p) (void)hipFree(p);
  delete arena;
  return PDSP_OK;
}

/* ---- device-pointer transforms --------------------------------------------- */

#define PDSP_DEFINE_TRANSFORMS(SUFFIX, T)                                                                          \
  int pdsp_fft_forward_real_##SUFFIX(const pdsp_plan *plan, long long batch, const T *re_in, T *re_out, T *im_out, \
                                     pdsp_stream stream) {                                                         \
    return run_complex<T>(plan, batch, re_in, nullptr, re_out, im_out, T(1), (hipStream_t)stream);                 \
  }                                                                                                                \
  int pdsp_fft_forward_complex_##SUFFIX(const pdsp_plan *plan, long long batch, const T *re_in, const T *im_in,    \
                                        T *re_out, T *im_out, pdsp_stream stream) {                                \
    if (batch > 0 && !im_in) return fail(PDSP_ERR_BAD_ARG, "null buffer");                                         \
    return run_complex<T>(plan, batch, re_in, im_in, re_out, im_out, T(1), (hipStream_t)stream);                   \
  }                                                                                                                \
  /* conj(FFT(conj(z))) == swap(FFT(swap(z))): the conjugated-twiddle sweep of fft.ts:122 is the forward */        \
  /* kernel with the planes exchanged on the way in and out; the 1/N of fft.ts:142-148 rides on the store */       \
  int pdsp_fft_inverse_##SUFFIX(const pdsp_plan *plan, long long batch, const T *re_in, const T *im_in, T *re_out, \
                                T *im_out, pdsp_stream stream) {                                                   \
    if (!plan) return fail(PDSP_ERR_BAD_ARG, "plan is null");                                                      \
    if (batch > 0 && !re_in) return fail(PDSP_ERR_BAD_ARG, "null buffer");                                         \
    return run_complex<T>(plan, batch, im_in, re_in, im_out, re_out, T(1) / (T)plan->n, (hipStream_t)stream);      \
  }                                                                                                                \
  int pdsp_fft_forward_interleaved_##SUFFIX(const pdsp_plan *plan, long long batch, const T *in, T *out,           \
                                            pdsp_stream stream) {                                                  \
    return run_interleaved<T>(plan, batch, in, out, false, (hipStream_t)stream);                                   \
  }                                                                                                                \
  int pdsp_fft_inverse_interleaved_##SUFFIX(const pdsp_plan *plan, long long batch, const T *in, T *out,           \
                                            pdsp_stream stream) {                                                  \
    return run_interleaved<T>(plan, batch, in, out, true, (hipStream_t)stream);                                    \
  }                                                                                                                \
  int pdsp_apply_window_##SUFFIX(long long batch, long long n, const T *in, const T *window, T *out,               \
                                 pdsp_stream stream) {                                                             \
    return apply_window_checked<T>(batch, n, in, window, out, (hipStream_t)stream);                                \
  }                                                                                                                \
  int pdsp_magnitude_##SUFFIX(long long count, const T *re, const T *im, T *out, pdsp_stream stream) {             \
    return polar_checked<T, false>(count, re, im, out, (hipStream_t)stream);                                       \
  }                                                                                                                \
  int pdsp_phase_##SUFFIX(long long count, const T *re, const T *im, T *out, pdsp_stream stream) {                 \
    return polar_checked<T, true>(count, re, im, out, (hipStream_t)stream);                                        \
  }                                                                                                                \
  int pdsp_spectrum_##SUFFIX(const pdsp_plan *plan, long long batch, const T *frames, long long frame_len,         \
                             long long frame_stride, const T *window, int sides, T *amp_out, T *phase_out,         \
                             int32_t *peak_out, pdsp_stream stream) {                                              \
    if (batch > 0 && !amp_out) return fail(PDSP_ERR_BAD_ARG, "null buffer");                                       \
    return spectrum_impl<T>(plan, batch, frames, frame_len, frame_stride, window, sides, amp_out, phase_out,       \
                            peak_out, nullptr, 1.0, (hipStream_t)stream);                                          \
  }

PDSP_DEFINE_TRANSFORMS(f32, float)
PDSP_DEFINE_TRANSFORMS(f64, double)
#undef PDSP_DEFINE_TRANSFORMS

int pdsp_complex_op_f32(int op, long long count, const float *a_re, const float *a_im, const float *b_re,
                        const float *b_im, long long b_len, double s_re, double s_im, float *out_re, float *out_im,
                        pdsp_stream stream) {
  if (count < 0) return fail(PDSP_ERR_BAD_ARG, "negative size");
  if (count > (LLONG_MAX / 8)) return fail(PDSP_ERR_BAD_ARG, "count %lld overflows", count);
  if (op < PDSP_CX_ADD || op > PDSP_CX_MUL_SCALAR) return fail(PDSP_ERR_BAD_ARG, "unknown complex op %d", op);
  if (count == 0) return PDSP_OK;
  if (!a_re || !a_im || !out_re || !out_im) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const bool binary = op <= PDSP_CX_DIV;
  if (binary) {
    if (!b_re || !b_im) return fail(PDSP_ERR_BAD_ARG, "null buffer");
    if (b_len <= 0 || count % b_len != 0)
      return fail(PDSP_ERR_BAD_ARG, "second operand length %lld must divide %lld", b_len, count);
  }
  // out may share bytes with a, or with a b of the same extent, only plane on plane (elementwise_clash): exact in
  // place, a == b == out, and out_re / out_im on a_im / a_re.  A broadcast b is read by every row: it shares nothing.
  const size_t bytes = (size_t)count * sizeof(float), b_bytes = (size_t)b_len * sizeof(float);
  const auto b_clash = [&](const float *o, const float *b) {
    return b_len == count ? elementwise_clash(o, b, bytes) : host_ranges_overlap(o, bytes, b, b_bytes);
  };
  bool clash = host_ranges_overlap(out_re, bytes, out_im, bytes);
  for (const float *o : {out_re, out_im}) {
    clash = clash || elementwise_clash(o, a_re, bytes) || elementwise_clash(o, a_im, bytes);
    if (binary) clash = clash || b_clash(o, b_re) || b_clash(o, b_im);
  }
  if (clash) return fail(PDSP_ERR_BAD_ARG, "output overlaps input");
  hipStream_t s = (hipStream_t)stream;
  const float sr = (float)s_re, si = (float)s_im;
  return complex_op_f32(op, count, a_re, a_im, b_re, b_im, b_len, sr, si, out_re, out_im, s);
}

/* ---- fused spectrum: peaks ---------------------------------------------------- */

int pdsp_spectrum_peaks_f32(const pdsp_plan *plan, long long batch, const float *frames, long long frame_len,
                            long long frame_stride, const float *window, int sides, double sample_rate,
                            float *amp_out, float *phase_out, pdsp_peak32 *peaks_out, pdsp_stream stream) {
  if (batch > 0 && !peaks_out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  return spectrum_impl<float>(plan, batch, frames, frame_len, frame_stride, window, sides, amp_out, phase_out, nullptr,
                              peaks_out, sample_rate, (hipStream_t)stream);
}

}  // extern "C"

/* ---- path queries of the entry points above ---------------------------------- */

int pdsp_dev_complex_op_vec4(int op, long long count, const float *a_re, const float *a_im, const float *b_re,
                             const float *b_im, long long b_len, const float *out_re, const float *out_im, int *vec4) {
  if (!vec4) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (op < PDSP_CX_ADD || op > PDSP_CX_MUL_SCALAR) return fail(PDSP_ERR_BAD_ARG, "unknown complex op %d", op);
  *vec4 = complex_op_vec4(op <= PDSP_CX_DIV, count, a_re, a_im, b_re, b_im, b_len, out_re, out_im);
  return PDSP_OK;
}

// The planes arrive in the public entry point's order: an inverse is run_complex on the exchanged planes, after
// pdsp_fft_inverse_*'s own checks
template <typename T>
static int transform_path_public(const pdsp_plan *plan, long long batch, const T *re_in, const T *im_in, const T *re_out,
                                 const T *im_out, int inverse, int *info) {
  if (!inverse) return transform_path<T>(plan, batch, re_in, im_in, re_out, im_out, info);
  if (!plan) return fail(PDSP_ERR_BAD_ARG, "plan is null");
  if (batch > 0 && !re_in) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  return transform_path<T>(plan, batch, im_in, re_in, im_out, re_out, info);
}
int pdsp_dev_transform_path_f32(const pdsp_plan *plan, long long batch, const float *re_in, const float *im_in,
                                const float *re_out, const float *im_out, int inverse, int info[PDSP_DEV_PATH_INFO]) {
  return transform_path_public<float>(plan, batch, re_in, im_in, re_out, im_out, inverse, info);
}
int pdsp_dev_transform_path_f64(const pdsp_plan *plan, long long batch, const double *re_in, const double *im_in,
                                const double *re_out, const double *im_out, int inverse, int info[PDSP_DEV_PATH_INFO]) {
  return transform_path_public<double>(plan, batch, re_in, im_in, re_out, im_out, inverse, info);
}
int pdsp_dev_spectrum_path_f32(const pdsp_plan *plan, long long batch, const float *frames, long long frame_len,
                               long long frame_stride, const float *window, int sides, const float *amp_out,
                               const float *phase_out, const int32_t *peak_idx_out, const pdsp_peak32 *peaks_out,
                               double sample_rate, int info[PDSP_DEV_PATH_INFO]) {
  return spectrum_path<float>(plan, batch, frames, frame_len, frame_stride, window, sides, amp_out, phase_out,
                              peak_idx_out, peaks_out, sample_rate, info);
}
int pdsp_dev_spectrum_path_f64(const pdsp_plan *plan, long long batch, const double *frames, long long frame_len,
                               long long frame_stride, const double *window, int sides, const double *amp_out,
                               const double *phase_out, const int32_t *peak_idx_out, const pdsp_peak32 *peaks_out,
                               double sample_rate, int info[PDSP_DEV_PATH_INFO]) {
  return spectrum_path<double>(plan, batch, frames, frame_len, frame_stride, window, sides, amp_out, phase_out,
                               peak_idx_out, peaks_out, sample_rate, info);
}

// pdsp_capi.hip -- the C ABI of include/pdsp_hip.h: argument validation with the
// reference's error texts, plan objects, kernel dispatch by size, and the
// synchronous host-f64 entry points the JS drop-in binds.
//
// Host side only, one of the library's translation units: no kernel is instantiated here (the dispatchers it
// calls -- run_complex, spectrum_impl, ... -- are declared in pdsp_internal.h and live in the
// pdsp_kernels_*.hip units).
//
// Product path only: nothing here touches oracle/, and there is no CPU fallback --
// without a HIP device every compute entry point fails with PDSP_ERR_DEVICE.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <climits>
#include <cstring>
#include <atomic>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "pdsp_internal.h"
#include "pdsp_goldilocks.h"

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

// Twiddle table for pdsp_radix.h's layout, built in f64 on the host
// (src/core/fft.ts:45-61 builds cos/sin of (-2*pi*k)/m per stage with Math.cos /
// Math.sin; same direct evaluation here, no recurrence), then rounded once.
template <typename T2>
std::vector<T2> build_twiddles(int log2n, int log2e = 4) {
  const pdsp::RadixPlan p = pdsp::make_radix_plan(log2n, log2e);
  std::vector<T2> tw((size_t)(p.twcount > 0 ? p.twcount : 1));
  for (int i = 0; i < p.np; ++i) {
    const int ns = p.ns[i], r = p.r[i];
    if (ns <= 1) continue;
    const double m = (double)ns * (double)r;
    for (int rr = 1; rr < r; ++rr)
      for (int k = 0; k < ns; ++k) {
        const double angle = (-2.0 * M_PI * (double)rr * (double)k) / m;
        T2 w;
        w.x = (decltype(w.x))std::cos(angle);
        w.y = (decltype(w.y))std::sin(angle);
        tw[(size_t)p.twoff[i] + (size_t)(rr - 1) * ns + k] = w;
      }
  }
  return tw;
}

// The plan's own stream, created on first use.  Caller holds plan->mu.
int ensure_plan_stream(pdsp_plan *plan) {
  if (!plan->stream) {
    PDSP_HIP_TRY(hipStreamCreateWithFlags(&plan->stream, hipStreamNonBlocking));
    ++g_live.streams;
  }
  return PDSP_OK;
}

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

// One-frame calls are latency-bound (two small copies + one kernel + one sync).  Up to 1 MiB of staging
// the kernel reads the frame from, and writes the result to, the pinned staging buffer itself
// (hipHostMalloc memory is mapped into the device's address space): no copy commands at all.
// PDSP_ZERO_COPY=0 in the environment restores the staged copies (A/B, tests); a value > 1 sets the limit.
long long g_zero_copy_bytes = -1;
bool zero_copy(size_t bytes) {
  if (g_zero_copy_bytes < 0) {
    const char *e = getenv("PDSP_ZERO_COPY");  // 0 = off, 1 / unset = default limit, > 1 = limit in bytes
    const long long v = e ? atoll(e) : 1;
    g_zero_copy_bytes = v <= 0 ? 0 : (v == 1 ? 1024 * 1024 : v);
  }
  return (long long)bytes <= g_zero_copy_bytes;
}
template <typename T>
T *stage_device_view(pdsp_plan *plan) {  // device-side address of the pinned staging buffer
  void *dp = nullptr;
  if (hipHostGetDevicePointer(&dp, plan->h_stage, 0) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return (T *)dp;
}

// Scratch (plan-less) staging for the element-wise host entry points.
template <typename T>
struct Scratch {
  T *h = nullptr, *d = nullptr;
  ~Scratch() {
    if (h) (void)hipHostFree(h);
    if (d) (void)hipFree(d);
  }
  int reserve(size_t count) {
    PDSP_HIP_TRY(hipHostMalloc((void **)&h, count * sizeof(T), hipHostMallocDefault));
    PDSP_HIP_TRY(hipMalloc((void **)&d, count * sizeof(T)));
    return PDSP_OK;
  }
};

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
struct PlanCache {
  struct Entry {
    pdsp_plan *plan = nullptr;
    unsigned long long last_use = 0;
    int pins = 0;
  };
  std::mutex mu;
  std::map<std::pair<long long, int>, Entry> plans;
  unsigned long long tick = 0;
};
PlanCache &plan_cache() {
  static PlanCache *c = new PlanCache();
  return *c;
}

// RAII pin of a cached plan for the duration of one host call.
struct CachedPlan {
  pdsp_plan *plan = nullptr;
  std::pair<long long, int> key{0, 0};
  CachedPlan() = default;
  CachedPlan(const CachedPlan &) = delete;
  CachedPlan &operator=(const CachedPlan &) = delete;
  ~CachedPlan() {
    if (!plan) return;
    PlanCache &c = plan_cache();
    std::lock_guard<std::mutex> lk(c.mu);
    auto it = c.plans.find(key);
    if (it != c.plans.end() && it->second.plan == plan) --it->second.pins;
  }
};

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

// The one place a plan table reaches the device: allocate, copy, record the allocation with its owner
// (Tables::release() frees that list, so a failure half way through a plan leaves nothing behind once the plan is
// released), store the pointer.  A failed copy frees its allocation at once: a retried plan_window does not pile up.
template <typename T, typename E, typename D>
hipError_t upload_table(Tables<T> &t, const std::vector<E> &host, D **out) {
  void *d = nullptr;
  if (hipError_t e = hipMalloc(&d, host.size() * sizeof(E))) return e;
  if (hipError_t e = hipMemcpy(d, host.data(), host.size() * sizeof(E), hipMemcpyHostToDevice)) {
    (void)hipFree(d);
    return e;
  }
  t.owned.push_back(d);
  t.owned_bytes += host.size() * sizeof(E);
  ++g_live.tables;
  g_live.table_bytes += (long long)(host.size() * sizeof(E));
  *out = (D *)d;
  return hipSuccess;
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

// Device copy of createWindow(type, N), built once per plan and precision (the window is
// always computed in f64 on the host and rounded once).  Caller holds plan->mu.
template <typename T>
int plan_window(pdsp_plan *plan, int type, const T **out) {
  Tables<T> &t = tables<T>(plan);
  if (!t.win[type]) {
    std::vector<double> w((size_t)plan->n);
    if (int rc = pdsp_window_make(type, plan->n, w.data())) return rc;
    if (hipError_t e = upload_table(t, std::vector<T>(w.begin(), w.end()), &t.win[type]))
      return fail(PDSP_ERR_DEVICE, "HIP error %d (%s) at hipMalloc / hipMemcpy of the window table", (int)e, hipGetErrorString(e));
  }
  *out = t.win[type];
  return PDSP_OK;
}

// Precision of the host-f64 entry points: 64 (default) computes in f64 wherever the single-pass
// kernels hold the size (complex N <= 8192, real spectrum N <= 16384) and in f32 beyond; 32 always
// computes in f32 (the north-star's contract).  PDSP_HOST_PRECISION=32 in the environment presets it.
int g_host_precision = 0;
int host_precision() {
  if (g_host_precision == 0) {
    const char *e = getenv("PDSP_HOST_PRECISION");
    g_host_precision = (e && atoi(e) == 32) ? 32 : 64;
  }
  return g_host_precision;
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

// ---- handles that own device tables -------------------------------------------------------------------------
// What the resampler, the DWT, the NTT, the sliding DFT and the chirp transforms share: a device, a lock, and the plans'
// own lists of allocations -- 4-byte tables in t32, 8-byte tables in t64 (the NTT's uint64_t roots among them) -- filled
// by upload_table and emptied by Tables::release, so a handle's tables are counted as a plan's are.  A handle adds what
// is its own, with its per-precision pointers behind one slot<T>().
struct TableHandle {
  int device = -1;  // < 0 until the first device call: the device current then
  std::mutex mu;    // the first-use upload; handles filled at create time never take it
  Tables<float> t32;
  Tables<double> t64;
  template <typename T>
  auto &owned() {
    if constexpr (sizeof(T) == 4) return t32;
    else return t64;
  }
};

// The device and the table of one call on stream s, for the handles whose table goes up on the first call in a
// precision (tap tables, root tables): under the handle's lock, the device resolved and current; where the slot is
// still empty, build() makes the host copy and it is uploaded -- unless s is being captured.  The one place a rule
// about lazy uploads has to be written.
template <typename T, class Build>
int first_use_table(TableHandle &h, T *&slot, hipStream_t s, const char *what, Build build) {
  std::lock_guard<std::mutex> lk(h.mu);
  if (int rc = resolve_device(&h.device)) return rc;
  DeviceGuard dg(h.device);
  PDSP_HIP_TRY(dg.err);
  if (slot) return PDSP_OK;
  if (int rc = refuse_upload_in_capture(s, what)) return rc;
  if (hipError_t e = upload_table(h.owned<T>(), build(), &slot))
    return fail(PDSP_ERR_DEVICE, "HIP error %d (%s) at hipMalloc / hipMemcpy of the %s", (int)e, hipGetErrorString(e),
                what);
  return PDSP_OK;
}

// A handle that owns no allocation (never used on a device, or its create failed at the first table) goes without a
// single HIP call: such handles are made and destroyed on machines with no device.
template <class H>
int destroy_handle(H *h) {
  if (!h) return PDSP_OK;
  if (!h->t32.owned.empty() || !h->t64.owned.empty()) {
    DeviceGuard g(h->device);
    h->t32.release();
    h->t64.release();
  }
  delete h;
  return PDSP_OK;
}

// The handle a host form makes for one call, destroyed on every exit.
template <class H>
struct HandleDeleter {
  void operator()(H *h) const { destroy_handle(h); }
};
template <class H>
using HandleOwner = std::unique_ptr<H, HandleDeleter<H>>;

// ---- chunked host calls -------------------------------------------------------------------------------------
// A batched host-f64 call moves every sample through the CPU twice (the caller's f64 rows <-> pinned staging), over
// PCIe twice, and through a kernel that needs a few percent of that time.  As ONE stage -> copy -> launch -> copy ->
// unstage sequence each step waits for the one before it and one core does all the staging: ~0.4 GSample/s at
// N = 4096 whatever the card does.  Calls above kChunkedMinBytes of staging are cut into chunks of ~kChunkInBytes of
// input rows instead; K workers (the calling thread and K - 1 helpers that live for the call) each own one staging
// slot and one stream and draw chunks from a shared counter: fill the slot, H2D, the same kernels the one-shot path
// launches, D2H, wait for the stream, unstage (+ findPeak).  Inside a worker the steps stay in order; across workers
// staging, both PCIe directions and the kernels overlap.  Row b of the result is the one-shot result of row b bit
// for bit, and the one-row call's on row b: the kernels work row by row, and the host forms choose the variant from
// the plan and the call's kind alone (run_complex with by_size; pick_spectrum never looks at the row count), so a
// chunk of any length, its shorter tail and a one-row call all run the same kernel on a row.  (Until the host forms
// passed by_size, f64 real rows of N = 16384 took fft_real_kernel from 8 rows per chunk up and the four-step path
// below: the bits depended on PDSP_HOST_THREADS, the core count and the batch.)  A worker keeps one
// chunk on the card while it fills the next (two slots and streams per worker).
// PDSP_HOST_THREADS sets K (1 = the one-shot sequence; default: half the cores this process may run on, 2 ... 6).
constexpr size_t kChunkInBytes = (size_t)2 << 20;
constexpr size_t kChunkedMinBytes = (size_t)4 << 20;
// Input bytes per chunk for a call that stages `in_total` bytes of input on `workers` workers: 2 MiB, less for small
// calls so that every worker still gets two chunks, not below 256 KiB.  (N = 1024 frames, us per call, one-shot /
// fixed 2-MiB chunks / these: 256 frames 327 / - / 304, 512 frames 597 / 445 / 406, 1,024 frames 1,331 / 652 / 536,
// 4,096 frames 14,663 / 1,405 / 1,527; 128 frames stay one-shot: 188 against 201.)
size_t chunk_in_bytes(size_t in_total, int workers) {
  size_t c = in_total / (size_t)(2 * (workers > 0 ? workers : 1));
  if (c > kChunkInBytes) c = kChunkInBytes;
  if (c < ((size_t)256 << 10)) c = (size_t)256 << 10;
  return c;
}

// multipass: the size runs on the multi-pass paths, whose scratch planes come from the engine's stream-ordered pool --
// planes freed on one stream are not reusable on another before a synchronisation, so many streams grow the pool
// through the driver instead of overlapping (f64 N = 16384 rows: 20 ms on 2 workers, 49-57 ms on 4-8): two workers.
int host_workers(bool multipass = false) {
  long v = 0;
  if (const char *e = getenv("PDSP_HOST_THREADS")) v = atol(e);
  if (v <= 0) {
    const unsigned hc = std::thread::hardware_concurrency();
    v = hc ? (long)(hc / 2) : 2;
    if (v < 2) v = 2;
    if (v > 6) v = 6;
  }
  if (multipass && v > 2) v = 2;
  return (int)(v > 16 ? 16 : v);
}

// How a batched host call is cut: rows per chunk and workers, or chunked = false for the one-shot sequence (which
// planes that overlap in host memory keep whatever this says).  pdsp_dev_host_*_chunks report it.
struct HostCut {
  bool chunked = false;
  long long per_chunk = 0;
  int workers = 0;
};
// pdsp_fft_transform_*host_f64 in precision T.  (Two planes' worth whether or not there is an imaginary input: the
// slot -- re | im | out re | out im -- stays at 2 x kChunkInBytes, so 2 slots x 6 workers fit the staging a plan
// keeps between calls.)
template <typename T>
HostCut transform_cut(const pdsp_plan *plan, long long batch) {
  const size_t row_bytes = (size_t)plan->n * sizeof(T), cnt = (size_t)batch * (size_t)plan->n;
  HostCut c;
  c.workers = host_workers(tables<T>(plan).log2n1 > 0);
  c.per_chunk = (long long)(chunk_in_bytes(2 * cnt * sizeof(T), c.workers) / (2 * row_bytes));
  c.chunked = c.workers >= 2 && c.per_chunk >= 1 && batch >= 2 * c.per_chunk && 4 * cnt * sizeof(T) >= kChunkedMinBytes;
  return c;
}
// pdsp_spectrum_*host_* on frames of len > 0 samples in precision T
template <typename T>
HostCut spectrum_cut(const pdsp_plan *plan, long long batch, long long bins) {
  const size_t frame_bytes = (size_t)plan->n * sizeof(T);
  HostCut c;
  c.workers = host_workers(tables<T>(plan).log2n1 > 0 && !tables<T>(plan).tw_half);  // packed-real frames: one pass
  c.per_chunk = (long long)(chunk_in_bytes((size_t)batch * frame_bytes, c.workers) / frame_bytes);
  c.chunked = c.workers >= 2 && c.per_chunk >= 1 && batch >= 2 * c.per_chunk &&
              (size_t)batch * (size_t)(plan->n + 2 * bins) * sizeof(T) >= kChunkedMinBytes;
  return c;
}

// One strided operand of a row call: rows of `len` elements, `stride` elements apart, `per_batch` of them for each row
// of the call (the sliding DFT's series: one per bin).  *count receives its extent in elements, from the first element
// of the first row to the last of the last: (rows - 1) * stride + len.
struct RowExtent {
  long long stride, len;
  long long *count;
  long long per_batch = 1;
};
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
// The host forms' twin: batch contiguous rows of len values, at most 2^40 of them (the caller words the refusal).
inline bool host_count_ok(long long batch, long long len, long long *count) {
  return mad_ok(batch, len, 0, count) && *count <= (1LL << 40);
}

// The element-wise kernels read index i of every input before they write index i and touch no other index, so an
// output may share bytes with an input of the same extent only where the two begin at the same address.
inline bool elementwise_clash(const void *out, const void *in, size_t bytes) {
  return out != in && host_ranges_overlap(out, bytes, in, bytes);
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

struct ChunkJob {
  long long first = 0, count = 0;  // rows [first, first + count) of the call
  int slot = 0;                    // staging slot of the worker that runs it
  hipStream_t stream = nullptr;
};

// submit(job) fills the job's slot and enqueues its copies and kernels on the job's stream without waiting;
// finish(job) is called after that stream has drained and unstages the results.  Both return a pdsp status (error
// text in the running thread's g_err).  Each worker owns TWO slots and streams and keeps one chunk on the card while
// it fills the next (slot = 2 * worker + parity), so the caller has staged 2 * `workers` slots (ensure_stage) and
// holds plan->mu.  The first failure stops the hand-out of chunks and is what the call returns.
constexpr int kSlotsPerWorker = 2;
template <class Submit, class Finish>
int run_chunked(pdsp_plan *plan, long long rows, long long rows_per_chunk, int workers, Submit submit, Finish finish) {
  const long long nchunks = (rows + rows_per_chunk - 1) / rows_per_chunk;
  if (workers > nchunks) workers = (int)nchunks;
  while ((long long)plan->slot_streams.size() < (long long)kSlotsPerWorker * workers) {
    hipStream_t st = nullptr;
    PDSP_HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    ++g_live.streams;
    plan->slot_streams.push_back(st);
  }
  std::atomic<long long> next{0};
  std::atomic<int> status{PDSP_OK};
  std::mutex err_mu;
  std::string err_text;
  auto report = [&](int rc) {
    std::lock_guard<std::mutex> lk(err_mu);
    if (status.load() == PDSP_OK) {
      err_text = g_err;
      status.store(rc);
    }
  };
  auto worker = [&](int w) {
    const hipError_t e = hipSetDevice(plan->device);  // helpers start on device 0
    if (e != hipSuccess) {
      report(fail(PDSP_ERR_DEVICE, "HIP error %d (%s) at hipSetDevice", (int)e, hipGetErrorString(e)));
      return;
    }
    ChunkJob in_flight;  // the chunk this worker has on the card (count == 0: none)
    auto complete = [&]() -> int {  // wait for the chunk in flight and unstage it
      if (in_flight.count == 0) return PDSP_OK;
      const hipError_t se = hipStreamSynchronize(in_flight.stream);
      int rc = PDSP_OK;
      if (se != hipSuccess) rc = fail(PDSP_ERR_DEVICE, "HIP error %d (%s) at hipStreamSynchronize", (int)se, hipGetErrorString(se));
      else rc = finish(in_flight);
      in_flight.count = 0;
      return rc;
    };
    int parity = 0;
    while (status.load() == PDSP_OK) {
      const long long c = next.fetch_add(1);
      if (c >= nchunks) break;
      ChunkJob job;
      job.first = c * rows_per_chunk;
      job.count = rows - job.first < rows_per_chunk ? rows - job.first : rows_per_chunk;
      job.slot = kSlotsPerWorker * w + parity;
      job.stream = plan->slot_streams[(size_t)job.slot];
      if (const int rc = submit(job)) {  // fills the OTHER slot while in_flight's chunk is on the card
        report(rc);
        break;
      }
      if (const int rc = complete()) {
        report(rc);
        in_flight = job;  // drained below
        break;
      }
      in_flight = job;
      parity ^= 1;
    }
    if (status.load() == PDSP_OK) {
      if (const int rc = complete()) report(rc);
    }
    // nothing of this call stays in flight on the worker's slots, on any exit
    for (int q = 0; q < kSlotsPerWorker; ++q) (void)hipStreamSynchronize(plan->slot_streams[(size_t)(kSlotsPerWorker * w + q)]);
  };
  std::vector<std::thread> helpers;
  helpers.reserve((size_t)workers);
  for (int w = 1; w < workers; ++w) {
    try {
      helpers.emplace_back(worker, w);
    } catch (...) {
      break;  // no more threads to be had: the workers that did start share the chunks
    }
  }
  worker(0);
  for (std::thread &t : helpers) t.join();
  if (status.load() != PDSP_OK) {
    g_err = err_text;
    return status.load();
  }
  return PDSP_OK;
}

// f64 staging copies INTO the pinned slots (the caller's rows -> slot) with non-temporal 16-byte stores: the destination
// lines are not read again by this core, so the read-for-ownership a plain store pays is pure host-memory traffic --
// and host memory traffic (48 bytes per sample between the staging copies and the DMA engines) is what bounds the
// chunked calls.  Measured, 6 workers: transforms +11 ... +15 %, spectrum at N = 4096 +11 ... +21 %, at N = 16384 +-0.
// The closing sfence orders the stores before the copy command that reads the slot.  PDSP_NT_COPY=0: plain memcpy.
inline bool nt_copy() {
  static const bool on = [] { const char *e = getenv("PDSP_NT_COPY"); return !(e && atoi(e) == 0); }();
  return on;
}
// `nt`: the chunked paths only -- a one-frame call's few KiB are read by its caller next, and should stay in cache.
inline void copy_f64(double *dst, const double *src, size_t count, bool nt) {
#if defined(__x86_64__)
  typedef double v2d __attribute__((vector_size(16), aligned(16)));
  typedef double v2du __attribute__((vector_size(16), aligned(8)));
  if (nt && nt_copy() && count >= 64 && !((uintptr_t)dst & 7) && !((uintptr_t)src & 7)) {
    size_t i = 0;
    if ((uintptr_t)dst & 15) dst[i] = src[i], ++i;
    for (; i + 2 <= count; i += 2) __builtin_nontemporal_store(*(const v2du *)(src + i), (v2d *)(dst + i));
    for (; i < count; ++i) dst[i] = src[i];
    __builtin_ia32_sfence();
    return;
  }
#endif
  std::memcpy(dst, src, count * sizeof(double));
}
template <typename T>
inline void rows_to_stage(T *dst, const double *src, size_t count, bool nt = false) {
  if constexpr (sizeof(T) == sizeof(double)) copy_f64(dst, src, count, nt);
  else
    for (size_t i = 0; i < count; ++i) dst[i] = (T)src[i];
}
// (results go out with ordinary stores: a caller's fresh result arrays are in cache right after their first touch,
// where a non-temporal store is the slower one; measured with reused arrays: no difference either way)
template <typename T>
inline void stage_to_rows(double *dst, const T *src, size_t count) {
  if constexpr (sizeof(T) == sizeof(double)) copy_f64(dst, src, count, false);
  else
    for (size_t i = 0; i < count; ++i) dst[i] = (double)src[i];
}

// Radix2Fft.transform for `batch` host rows in precision T (f64 at the boundary either way).  Input rows either
// contiguous (re_in / im_in) or one pointer per row (re_rows / im_rows: pdsp_fft_transform_rows_host_f64).
template <typename T>
int transform_host(pdsp_plan *plan, long long batch, const double *re_in, const double *im_in,
                   const double *const *re_rows, const double *const *im_rows, double *re_out, double *im_out,
                   int inverse) {
  const size_t n = (size_t)plan->n, cnt = (size_t)batch * n;
  const bool has_im = im_in || im_rows;
  auto re_row = [&](long long r) { return re_rows ? re_rows[r] : re_in + (size_t)r * n; };
  auto im_row = [&](long long r) { return im_rows ? im_rows[r] : im_in + (size_t)r * n; };
  // rows [first, first + count) into staging planes of `count` rows each
  auto stage_in = [&](T *h_re, T *h_im, long long first, long long count, bool nt) {
    if (!re_rows) rows_to_stage<T>(h_re, re_in + (size_t)first * n, (size_t)count * n, nt);
    else
      for (long long r = 0; r < count; ++r) rows_to_stage<T>(h_re + (size_t)r * n, re_rows[first + r], n, nt);
    if (!has_im) return;
    if (!im_rows) rows_to_stage<T>(h_im, im_in + (size_t)first * n, (size_t)count * n, nt);
    else
      for (long long r = 0; r < count; ++r) rows_to_stage<T>(h_im + (size_t)r * n, im_rows[first + r], n, nt);
  };
  {
    // many rows: chunks on several workers (run_chunked); planes that overlap each other in host memory keep the
    // one-shot sequence, which has read every input before it writes any output
    const size_t out_bytes = cnt * sizeof(double), in_row_bytes = n * sizeof(double);
    const HostCut cut = transform_cut<T>(plan, batch);
    const int workers = cut.workers;
    const long long per_chunk = cut.per_chunk;
    bool overlap = false;
    if (re_rows || im_rows) {
      for (long long r = 0; r < batch && !overlap; ++r)
        overlap = host_ranges_overlap(re_row(r), in_row_bytes, re_out, out_bytes) ||
                  host_ranges_overlap(re_row(r), in_row_bytes, im_out, out_bytes) ||
                  (has_im && (host_ranges_overlap(im_row(r), in_row_bytes, re_out, out_bytes) ||
                              host_ranges_overlap(im_row(r), in_row_bytes, im_out, out_bytes)));
    } else {
      overlap = host_ranges_overlap(re_in, out_bytes, re_out, out_bytes) || host_ranges_overlap(re_in, out_bytes, im_out, out_bytes) ||
                host_ranges_overlap(im_in, out_bytes, re_out, out_bytes) || host_ranges_overlap(im_in, out_bytes, im_out, out_bytes);
    }
    if (cut.chunked && !overlap) {
      const size_t slot = 4 * (size_t)per_chunk * n;  // elements: re | im | out re | out im
      const int k = (long long)workers < (batch + per_chunk - 1) / per_chunk ? workers : (int)((batch + per_chunk - 1) / per_chunk);
      if (int rc = ensure_stage(plan, (size_t)kSlotsPerWorker * k * slot * sizeof(T))) return rc;
      return run_chunked(
          plan, batch, per_chunk, k,
          [&](const ChunkJob &job) -> int {  // submit
            const size_t c = (size_t)job.count * n;
            T *h = (T *)plan->h_stage + (size_t)job.slot * slot, *d = (T *)plan->d_stage + (size_t)job.slot * slot;
            stage_in(h, h + c, job.first, job.count, true);
            PDSP_HIP_TRY(hipMemcpyAsync(d, h, (has_im ? 2 : 1) * c * sizeof(T), hipMemcpyHostToDevice, job.stream));
            int rc;
            // by_size: a chunk's row count must not choose the kernel (see above kChunkInBytes)
            if (inverse) rc = run_complex<T>(plan, job.count, d + c, d, d + 3 * c, d + 2 * c, T(1) / (T)plan->n, job.stream, true);
            else rc = run_complex<T>(plan, job.count, d, has_im ? d + c : nullptr, d + 2 * c, d + 3 * c, T(1), job.stream, true);
            if (rc) return rc;
            PDSP_HIP_TRY(hipMemcpyAsync(h + 2 * c, d + 2 * c, 2 * c * sizeof(T), hipMemcpyDeviceToHost, job.stream));
            return PDSP_OK;
          },
          [&](const ChunkJob &job) -> int {  // finish
            const size_t c = (size_t)job.count * n, off = (size_t)job.first * n;
            const T *h = (const T *)plan->h_stage + (size_t)job.slot * slot;
            stage_to_rows<T>(re_out + off, h + 2 * c, c);
            stage_to_rows<T>(im_out + off, h + 3 * c, c);
            return PDSP_OK;
          });
    }
  }
  if (int rc = ensure_stage(plan, 4 * cnt * sizeof(T))) return rc;
  T *h_re = (T *)plan->h_stage, *h_im = h_re + cnt, *h_ore = h_im + cnt, *h_oim = h_ore + cnt;
  T *d_re = (T *)plan->d_stage, *d_im = d_re + cnt, *d_ore = d_im + cnt, *d_oim = d_ore + cnt;
  stage_in(h_re, h_im, 0, batch, false);
  hipStream_t s = plan->stream;
  T *const z = zero_copy(4 * cnt * sizeof(T)) ? stage_device_view<T>(plan) : nullptr;
  if (z) {  // the kernels work on the pinned buffer itself
    d_re = z, d_im = z + cnt, d_ore = z + 2 * cnt, d_oim = z + 3 * cnt;
  } else {
    PDSP_HIP_TRY(hipMemcpyAsync(d_re, h_re, (has_im ? 2 : 1) * cnt * sizeof(T), hipMemcpyHostToDevice, s));
  }
  int rc;
  // inverse: conj(FFT(conj(z))) == swap(FFT(swap(z))) -- the conjugated-twiddle sweep of fft.ts:122
  // is the forward kernel with the planes exchanged on the way in and out; 1/N rides on the store
  if (inverse) rc = run_complex<T>(plan, batch, d_im, d_re, d_oim, d_ore, T(1) / (T)plan->n, s, true);
  else rc = run_complex<T>(plan, batch, d_re, has_im ? d_im : nullptr, d_ore, d_oim, T(1), s, true);
  if (rc) return rc;
  if (!z) PDSP_HIP_TRY(hipMemcpyAsync(h_ore, d_ore, 2 * cnt * sizeof(T), hipMemcpyDeviceToHost, s));
  PDSP_HIP_TRY(hipStreamSynchronize(s));
  stage_to_rows<T>(re_out, h_ore, cnt);
  stage_to_rows<T>(im_out, h_oim, cnt);
  return PDSP_OK;
}

template <typename T>
int apply_window_host(const double *in, long long n_, const double *window, double *out) {
  Scratch<T> sc;
  const size_t n = (size_t)n_;
  if (int rc = sc.reserve(3 * n)) return rc;
  for (size_t i = 0; i < n; ++i) sc.h[i] = (T)in[i];
  for (size_t i = 0; i < n; ++i) sc.h[n + i] = (T)window[i];
  PDSP_HIP_TRY(hipMemcpy(sc.d, sc.h, 2 * n * sizeof(T), hipMemcpyHostToDevice));
  if (int rc = apply_window_dev<T>(1, n_, sc.d, sc.d + n, sc.d + 2 * n, nullptr)) return rc;
  PDSP_HIP_TRY(hipMemcpy(sc.h, sc.d + 2 * n, n * sizeof(T), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) out[i] = (double)sc.h[i];
  return PDSP_OK;
}

template <typename T>
int polar_host_t(const double *re, const double *im, long long n_, double *out, bool want_phase) {
  Scratch<T> sc;
  const size_t n = (size_t)n_;
  if (int rc = sc.reserve(3 * n)) return rc;
  for (size_t i = 0; i < n; ++i) sc.h[i] = (T)re[i];
  for (size_t i = 0; i < n; ++i) sc.h[n + i] = (T)im[i];
  PDSP_HIP_TRY(hipMemcpy(sc.d, sc.h, 2 * n * sizeof(T), hipMemcpyHostToDevice));
  const int rc = want_phase ? polar_dev<T, true>(n_, sc.d, sc.d + n, sc.d + 2 * n, nullptr)
                            : polar_dev<T, false>(n_, sc.d, sc.d + n, sc.d + 2 * n, nullptr);
  if (rc) return rc;
  PDSP_HIP_TRY(hipMemcpy(sc.h, sc.d + 2 * n, n * sizeof(T), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; ++i) out[i] = (double)sc.h[i];
  return PDSP_OK;
}

// `batch` frames of spectrum() (each `len` samples, contiguous) in precision T; plan->mu held by the
// caller.  One frame (the drop-in spectrum()) and many (spectrumBatch) run the same kernel variant per
// row, so row b of a batch equals the one-frame call on frame b bit for bit.
// findPeak on the host over `count` rows of f64 amplitudes: exact strict-'>' and first-wins
// behaviour (spectrum.ts:74-105), peak.frequency from the call's one frequency axis.
inline void host_peaks(const double *freq, const double *amp_rows, const double *phase_rows, long long bins,
                       long long count, pdsp_peak *peak_out) {
  for (long long b = 0; b < count; ++b) {
    const double *a = amp_rows + (size_t)b * (size_t)bins, *p = phase_rows + (size_t)b * (size_t)bins;
    const long long pk = pdsp_find_peak_f64(a, bins);
    peak_out[b].index = (int32_t)pk;
    peak_out[b].frequency = freq[pk];
    peak_out[b].amplitude = a[pk];
    peak_out[b].phase = p[pk];
  }
}

// Where the frames of a host spectrum call lie: contiguous f64 (pdsp_spectrum_batch_host_f64), one pointer per frame
// in f64 (pdsp_spectrum_rows_host_f64) or in f32 (pdsp_spectrum_rows_host_f32in: Float32Array audio frames).
struct FrameSource {
  const double *samples = nullptr;
  const double *const *rows64 = nullptr;
  const float *const *rows32 = nullptr;
  long long len = 0;
  size_t frame_bytes() const { return (size_t)len * (rows32 ? sizeof(float) : sizeof(double)); }
  const void *frame(long long b) const {
    if (rows32) return rows32[b];
    return rows64 ? rows64[b] : samples + (size_t)b * (size_t)len;
  }
  // the first `used` samples of frame b into staging of precision T
  template <typename T>
  void stage(T *dst, long long b, size_t used, bool nt = false) const {
    if (rows32) {
      const float *src = rows32[b];
      if constexpr (sizeof(T) == sizeof(float)) std::memcpy(dst, src, used * sizeof(float));
      else
        for (size_t i = 0; i < used; ++i) dst[i] = (T)src[i];
    } else {
      rows_to_stage<T>(dst, (const double *)frame(b), used, nt);
    }
  }
  bool overlaps(const void *out, size_t out_bytes, long long batch) const {
    if (!rows64 && !rows32) return host_ranges_overlap(samples, (size_t)batch * frame_bytes(), out, out_bytes);
    for (long long b = 0; b < batch; ++b)
      if (host_ranges_overlap(frame(b), frame_bytes(), out, out_bytes)) return true;
    return false;
  }
};

template <typename T>
int spectrum_host_t(pdsp_plan *plan, const FrameSource &in, int window, int sides, double *amp_out, double *phase_out,
                    long long batch, const double *freq, pdsp_peak *peak_out) {
  const long long len = in.len;
  const long long n = plan->n;
  const long long bins = sides == PDSP_SIDES_ONE ? n / 2 + 1 : n;
  const long long used = len < n ? len : n;
  {
    // many frames: chunks on several workers (run_chunked)
    const size_t frame_bytes = (size_t)n * sizeof(T);
    const HostCut cut = spectrum_cut<T>(plan, batch, bins);
    const int workers = cut.workers;
    const long long per_chunk = cut.per_chunk;
    const size_t out_b = (size_t)batch * (size_t)bins * sizeof(double);
    const bool overlap = len > 0 && (in.overlaps(amp_out, out_b, batch) || in.overlaps(phase_out, out_b, batch));
    if (cut.chunked && len > 0 && !overlap) {
      const T *d_window = nullptr;
      if (n != 1 && window != PDSP_WIN_RECT) {
        if (int rc = plan_window<T>(plan, window, &d_window)) return rc;  // built once, before the workers read it
      }
      // slot (elements): [per_chunk frames of n][per_chunk rows of amp][per_chunk rows of phase], 16-byte aligned parts
      const size_t amp_off = ((size_t)per_chunk * (size_t)n + 3) & ~(size_t)3;
      const size_t ph_off = (amp_off + (size_t)per_chunk * (size_t)bins + 3) & ~(size_t)3;
      const size_t slot = (ph_off + (size_t)per_chunk * (size_t)bins + 3) & ~(size_t)3;
      const long long nchunks = (batch + per_chunk - 1) / per_chunk;
      const int k = (long long)workers < nchunks ? workers : (int)nchunks;
      if (int rc = ensure_stage(plan, (size_t)kSlotsPerWorker * k * slot * sizeof(T))) return rc;
      return run_chunked(
          plan, batch, per_chunk, k,
          [&](const ChunkJob &job) -> int {  // submit
            T *h = (T *)plan->h_stage + (size_t)job.slot * slot, *d = (T *)plan->d_stage + (size_t)job.slot * slot;
            for (long long b = 0; b < job.count; ++b) {
              T *dst = h + (size_t)b * (size_t)n;
              in.stage<T>(dst, job.first + b, (size_t)used, true);
              if (used < n) std::memset(dst + used, 0, (size_t)(n - used) * sizeof(T));
            }
            const size_t rows = (size_t)job.count * (size_t)bins;
            PDSP_HIP_TRY(hipMemcpyAsync(d, h, (size_t)job.count * frame_bytes, hipMemcpyHostToDevice, job.stream));
            if (int rc = spectrum_impl<T>(plan, job.count, d, n, n, d_window, sides, d + amp_off, d + ph_off, nullptr,
                                          nullptr, 1.0, job.stream))
              return rc;
            PDSP_HIP_TRY(hipMemcpyAsync(h + amp_off, d + amp_off, rows * sizeof(T), hipMemcpyDeviceToHost, job.stream));
            PDSP_HIP_TRY(hipMemcpyAsync(h + ph_off, d + ph_off, rows * sizeof(T), hipMemcpyDeviceToHost, job.stream));
            return PDSP_OK;
          },
          [&](const ChunkJob &job) -> int {  // finish
            const T *h = (const T *)plan->h_stage + (size_t)job.slot * slot;
            const size_t rows = (size_t)job.count * (size_t)bins;
            // (host_peaks below reads the f64 rows from the slot, which is still in cache, not from the rows just streamed out)
            stage_to_rows<T>(amp_out + (size_t)job.first * (size_t)bins, h + amp_off, rows);
            stage_to_rows<T>(phase_out + (size_t)job.first * (size_t)bins, h + ph_off, rows);
            if (peak_out) {
              if constexpr (sizeof(T) == sizeof(double))
                host_peaks(freq, (const double *)(h + amp_off), (const double *)(h + ph_off), bins, job.count, peak_out + job.first);
              else
                host_peaks(freq, amp_out + (size_t)job.first * (size_t)bins, phase_out + (size_t)job.first * (size_t)bins, bins,
                           job.count, peak_out + job.first);
            }
            return PDSP_OK;
          });
    }
  }
  // staging: [batch frames of n][batch rows of amp][batch rows of phase]; rows start 16-byte aligned
  const size_t rows = (size_t)batch * (size_t)bins, frames_sz = (size_t)batch * (size_t)n;
  const size_t amp_off = (frames_sz + 3) & ~(size_t)3, ph_off = (amp_off + rows + 3) & ~(size_t)3;
  const size_t total = ph_off + rows;
  if (int rc = ensure_stage(plan, total * sizeof(T))) return rc;
  T *h = (T *)plan->h_stage, *d = (T *)plan->d_stage;
  for (long long b = 0; b < batch; ++b) {
    T *dst = h + (size_t)b * (size_t)n;
    if (used > 0) in.stage<T>(dst, b, (size_t)used);
    for (long long i = used; i < n; ++i) dst[i] = T(0);
  }
  const T *d_window = nullptr;
  if (n != 1 && window != PDSP_WIN_RECT) {
    if (int rc = plan_window<T>(plan, window, &d_window)) return rc;
  }
  hipStream_t s = plan->stream;
  T *const z = zero_copy(total * sizeof(T)) ? stage_device_view<T>(plan) : nullptr;
  if (z) d = z;  // the kernel works on the pinned buffer itself
  else PDSP_HIP_TRY(hipMemcpyAsync(d, h, frames_sz * sizeof(T), hipMemcpyHostToDevice, s));
  if (int rc = spectrum_impl<T>(plan, batch, d, n, n, d_window, sides, d + amp_off, d + ph_off, nullptr, nullptr, 1.0, s))
    return rc;
  if (!z) PDSP_HIP_TRY(hipMemcpyAsync(h + amp_off, d + amp_off, (total - amp_off) * sizeof(T), hipMemcpyDeviceToHost, s));
  PDSP_HIP_TRY(hipStreamSynchronize(s));
  for (size_t i = 0; i < rows; ++i) amp_out[i] = (double)h[amp_off + i];
  for (size_t i = 0; i < rows; ++i) phase_out[i] = (double)h[ph_off + i];
  if (peak_out) host_peaks(freq, amp_out, phase_out, bins, batch, peak_out);
  return PDSP_OK;
}

int spectrum_frames_host(const FrameSource &in, long long batch, double sample_rate, long long fft_size, int window,
                         int sides, double *freq_out, double *amp_out, double *phase_out, pdsp_peak *peak_out,
                         long long *bins_out);

}  // namespace

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

int pdsp_set_host_precision(int bits) {
  const int prev = host_precision();
  if (bits == 32 || bits == 64) g_host_precision = bits;
  return prev;
}

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

/* ---- host f64 drop-in entry points ------------------------------------------ */

int pdsp_fft_transform_host_f64(pdsp_plan *plan, long long batch, long long in_len, const double *re_in,
                                const double *im_in, double *re_out, double *im_out, int inverse) {
  if (int rc = check_plan_batch(plan, batch)) return rc;
  if (in_len != plan->n) return fail(PDSP_ERR_INPUT_LENGTH, "FFT input length %lld != size %lld", in_len, plan->n);
  if (batch == 0) return PDSP_OK;
  if (!re_in || !re_out || !im_out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (inverse && !im_in) return fail(PDSP_ERR_BAD_ARG, "inverse needs an imaginary plane");
  std::lock_guard<std::mutex> lk(plan->mu);
  DeviceGuard g(plan->device);
  PDSP_HIP_TRY(g.err);
  const int rc = (host_precision() == 64 && plan->t64.tw)
                     ? transform_host<double>(plan, batch, re_in, im_in, nullptr, nullptr, re_out, im_out, inverse)
                     : transform_host<float>(plan, batch, re_in, im_in, nullptr, nullptr, re_out, im_out, inverse);
  trim_stage(plan);
  return rc;
}

int pdsp_fft_transform_rows_host_f64(pdsp_plan *plan, long long batch, long long in_len, const double *const *re_rows,
                                     const double *const *im_rows, double *re_out, double *im_out, int inverse) {
  if (int rc = check_plan_batch(plan, batch)) return rc;
  if (in_len != plan->n) return fail(PDSP_ERR_INPUT_LENGTH, "FFT input length %lld != size %lld", in_len, plan->n);
  if (batch == 0) return PDSP_OK;
  if (!re_rows || !re_out || !im_out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (inverse && !im_rows) return fail(PDSP_ERR_BAD_ARG, "inverse needs an imaginary plane");
  for (long long r = 0; r < batch; ++r)
    if (!re_rows[r] || (im_rows && !im_rows[r])) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  std::lock_guard<std::mutex> lk(plan->mu);
  DeviceGuard g(plan->device);
  PDSP_HIP_TRY(g.err);
  const int rc = (host_precision() == 64 && plan->t64.tw)
                     ? transform_host<double>(plan, batch, nullptr, nullptr, re_rows, im_rows, re_out, im_out, inverse)
                     : transform_host<float>(plan, batch, nullptr, nullptr, re_rows, im_rows, re_out, im_out, inverse);
  trim_stage(plan);
  return rc;
}

int pdsp_apply_window_host_f64(const double *in, long long in_len, const double *window, long long window_len,
                               double *out) {
  if (in_len != window_len) return fail(PDSP_ERR_WINDOW_LENGTH, "Window length must match input length.");
  if (in_len == 0) return PDSP_OK;
  if (in_len < 0 || !in || !window || !out) return fail(PDSP_ERR_BAD_ARG, "bad applyWindow arguments");
  if (int rc = require_device()) return rc;
  return host_precision() == 64 ? apply_window_host<double>(in, in_len, window, out)
                                : apply_window_host<float>(in, in_len, window, out);
}

static int polar_host(const double *re, const double *im, long long n, double *out, bool want_phase) {
  if (n == 0) return PDSP_OK;
  if (n < 0 || !re || !im || !out) return fail(PDSP_ERR_BAD_ARG, "bad magnitude/phase arguments");
  if (int rc = require_device()) return rc;
  return host_precision() == 64 ? polar_host_t<double>(re, im, n, out, want_phase)
                                : polar_host_t<float>(re, im, n, out, want_phase);
}

int pdsp_magnitude_host_f64(const double *re, const double *im, long long n, double *out) {
  return polar_host(re, im, n, out, false);
}

int pdsp_phase_host_f64(const double *re, const double *im, long long n, double *out) {
  return polar_host(re, im, n, out, true);
}

int pdsp_spectrum_host_f64(const double *samples, long long len, double sample_rate, long long fft_size, int window,
                           int sides, double *freq_out, double *amp_out, double *phase_out, pdsp_peak *peak_out,
                           long long *bins_out) {
  return pdsp_spectrum_batch_host_f64(samples, 1, len, sample_rate, fft_size, window, sides, freq_out, amp_out, phase_out,
                                      peak_out, bins_out);
}

int pdsp_spectrum_batch_host_f64(const double *samples, long long batch, long long len, double sample_rate,
                                 long long fft_size, int window, int sides, double *freq_out, double *amp_out,
                                 double *phase_out, pdsp_peak *peak_out, long long *bins_out) {
  if (len > 0 && batch > 0 && !samples) return fail(PDSP_ERR_BAD_ARG, "bad samples");
  FrameSource in;
  in.samples = samples;
  in.len = len;
  return spectrum_frames_host(in, batch, sample_rate, fft_size, window, sides, freq_out, amp_out, phase_out, peak_out,
                              bins_out);
}

int pdsp_spectrum_rows_host_f64(const double *const *rows, long long batch, long long len, double sample_rate,
                                long long fft_size, int window, int sides, double *freq_out, double *amp_out,
                                double *phase_out, pdsp_peak *peak_out, long long *bins_out) {
  if (batch > 0 && len > 0) {
    if (!rows) return fail(PDSP_ERR_BAD_ARG, "bad samples");
    for (long long b = 0; b < batch; ++b)
      if (!rows[b]) return fail(PDSP_ERR_BAD_ARG, "bad samples");
  }
  FrameSource in;
  in.rows64 = len > 0 ? rows : nullptr;
  in.len = len;
  return spectrum_frames_host(in, batch, sample_rate, fft_size, window, sides, freq_out, amp_out, phase_out, peak_out,
                              bins_out);
}

int pdsp_spectrum_rows_host_f32in(const float *const *rows, long long batch, long long len, double sample_rate,
                                  long long fft_size, int window, int sides, double *freq_out, double *amp_out,
                                  double *phase_out, pdsp_peak *peak_out, long long *bins_out) {
  if (batch > 0 && len > 0) {
    if (!rows) return fail(PDSP_ERR_BAD_ARG, "bad samples");
    for (long long b = 0; b < batch; ++b)
      if (!rows[b]) return fail(PDSP_ERR_BAD_ARG, "bad samples");
  }
  FrameSource in;
  in.rows32 = len > 0 ? rows : nullptr;
  in.len = len;
  return spectrum_frames_host(in, batch, sample_rate, fft_size, window, sides, freq_out, amp_out, phase_out, peak_out,
                              bins_out);
}

}  // extern "C"

namespace {

int spectrum_frames_host(const FrameSource &in, long long batch, double sample_rate, long long fft_size, int window,
                         int sides, double *freq_out, double *amp_out, double *phase_out, pdsp_peak *peak_out,
                         long long *bins_out) {
  const long long len = in.len;
  if (batch < 0) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 0, got %lld", batch);
  if (len < 0) return fail(PDSP_ERR_BAD_ARG, "bad samples");
  if (sides != PDSP_SIDES_ONE && sides != PDSP_SIDES_TWO) return fail(PDSP_ERR_BAD_ARG, "bad sides %d", sides);
  // Error order of spectrum.ts:113-132: FFT ctor (power of two) -> createWindow
  // (type; N == 1 returns before the type switch) -> ... -> binFrequencies (rate).
  const long long n = fft_size >= 0 ? fft_size : pdsp_next_pow2(len);  // < 0: options.fftSize absent
  if (!pdsp_is_pow2(n)) return fail(PDSP_ERR_SIZE_NOT_POW2, "FFT size must be power of two, got %lld", n);
  if (n != 1 && (window < PDSP_WIN_RECT || window > PDSP_WIN_BLACKMAN))
    return fail(PDSP_ERR_WINDOW_TYPE, "Unsupported window type: %d", window);
  if (sample_rate <= 0) return fail(PDSP_ERR_SAMPLE_RATE, "Sample rate must be positive, got %.17g", sample_rate);
  if (!freq_out || !amp_out || !phase_out) return fail(PDSP_ERR_BAD_ARG, "null output");
  if (int rc = require_device()) return rc;
  CachedPlan pin;
  if (int rc = cached_plan(n, &pin)) return rc;  // plan + window are cached per (size, device), LRU-bounded
  pdsp_plan *const plan = pin.plan;
  std::lock_guard<std::mutex> lk(plan->mu);
  DeviceGuard g(plan->device);
  PDSP_HIP_TRY(g.err);
  const long long bins = sides == PDSP_SIDES_ONE ? n / 2 + 1 : n;
  if (int rc = pdsp_bin_frequencies(n, sample_rate, sides, freq_out, nullptr)) return rc;
  if (bins_out) *bins_out = bins;
  if (batch == 0) return PDSP_OK;
  const bool f64 = host_precision() == 64 && (plan->t64.tw_half || plan->t64.tw);
  // (len == 0: every frame is all zero padding; no frame is read)
  // findPeak runs on the host over the f64 amplitudes (host_peaks), inside the call's staging loop
  const int rc_run = f64 ? spectrum_host_t<double>(plan, in, window, sides, amp_out, phase_out, batch, freq_out, peak_out)
                         : spectrum_host_t<float>(plan, in, window, sides, amp_out, phase_out, batch, freq_out, peak_out);
  trim_stage(plan);
  return rc_run;
}

}  // namespace

/* ---- FIR filtering: fused overlap-save --------------------------------------- */

namespace pdsp_host {

// The packed-real kernels (FIR filtering, the short-time pair, the DCT) run on the N/2-point tables, N = 64 ... 16384
// in both precisions; the DCT also on W_4N^k.  `what` names the feature in the error text.
int packed_size_error(const char *what, long long n) {
  return fail(PDSP_ERR_UNSUPPORTED_SIZE, "%s needs a plan of 64 <= N <= 16384, got %lld", what, n);
}
template <typename T>
int check_packed_plan(const pdsp_plan *plan, const char *what, bool need_tw4n) {
  if (!plan) return fail(PDSP_ERR_BAD_ARG, "plan is null");
  const Tables<T> &t = tables<T>(plan);
  if (plan->log2n < 6 || plan->log2n > pdsp::kMaxLog2N_f32 || !t.tw_half || !t.twr || (need_tw4n && !t.tw4n))
    return packed_size_error(what, plan->n);
  return PDSP_OK;
}

// The same gate for the bare size of a host form, behind the power-of-two check of the plan it will ask for.
int check_packed_size(long long n, const char *what) {
  if (!pdsp_is_pow2(n)) return fail(PDSP_ERR_SIZE_NOT_POW2, "FFT size must be power of two, got %lld", n);
  if (n < 64 || n > 16384) return packed_size_error(what, n);
  return PDSP_OK;
}

// Device memory of one host call, freed on every exit.
struct DeviceBuf {
  double *d = nullptr;
  ~DeviceBuf() {
    if (d) (void)hipFree(d);
  }
};

// What the stream-ordered host forms of the packed features share, behind their own argument checks: the cached plan
// of `n` points, pinned and locked for the call, with its device current; the plan's f64 window unless the type is
// rect; one device buffer of `count` values.  enqueue(plan, stream, window, buffer) lays the buffer out, enqueues the
// copies in and the call on the plan's stream; collect(buffer) copies the results out once that stream has drained.
// (One explicit stream for every step: the two-pass ISTFT draws its scratch stream-ordered, StreamScratch.)
template <class Enqueue, class Collect>
int packed_host_call(long long n, int window_type, size_t count, Enqueue enqueue, Collect collect) {
  if (int rc = require_device()) return rc;
  CachedPlan cp;
  if (int rc = cached_plan(n, &cp)) return rc;
  pdsp_plan *const plan = cp.plan;
  std::lock_guard<std::mutex> lk(plan->mu);
  DeviceGuard g(plan->device);
  PDSP_HIP_TRY(g.err);
  const double *win = nullptr;
  if (window_type != PDSP_WIN_RECT)
    if (int rc = plan_window<double>(plan, window_type, &win)) return rc;
  if (int rc = ensure_plan_stream(plan)) return rc;
  DeviceBuf buf;
  PDSP_HIP_TRY(hipMalloc((void **)&buf.d, count * sizeof(double)));
  if (int rc = enqueue(plan, plan->stream, win, buf.d)) return rc;
  PDSP_HIP_TRY(hipStreamSynchronize(plan->stream));
  return collect(buf.d);
}

// Filters have at most N/2 taps (the tap count is checked ahead of the plan's size, behind its null check).
template <typename T>
int check_fir_plan(const pdsp_plan *plan, long long ntaps) {
  if (plan && ntaps < 1) return fail(PDSP_ERR_BAD_ARG, "filter must have at least one tap, got %lld", ntaps);
  if (int rc = check_packed_plan<T>(plan, "FIR filtering", false)) return rc;
  if (ntaps > plan->n / 2)
    return fail(PDSP_ERR_UNSUPPORTED_SIZE, "filter of %lld taps exceeds N/2 = %lld of the plan (no partitioned convolution)",
                ntaps, plan->n / 2);
  return PDSP_OK;
}

template <typename T>
int fir_spectrum_t(const pdsp_plan *plan, const T *taps, long long ntaps, T *h_re, T *h_im, hipStream_t s) {
  if (int rc = check_fir_plan<T>(plan, ntaps)) return rc;
  if (!taps || !h_re || !h_im) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  DeviceGuard g(plan->device);
  PDSP_HIP_TRY(g.err);
  return fir_spectrum_dev<T>(plan, taps, (int)ntaps, h_re, h_im, s);
}

template <typename T>
int fir_filter_t(const pdsp_plan *plan, long long batch, const T *x, long long len, long long x_stride, const T *h_re,
                 const T *h_im, long long ntaps, long long y_off, long long y_len, T *y, long long y_stride,
                 hipStream_t s) {
  if (int rc = check_fir_plan<T>(plan, ntaps)) return rc;
  if (batch < 0 || len < 0 || y_off < 0 || y_len < 0)
    return fail(PDSP_ERR_BAD_ARG, "negative size (batch %lld, len %lld, y_off %lld, y_len %lld)", batch, len, y_off, y_len);
  if (x_stride < 0 || y_stride < 0) return fail(PDSP_ERR_BAD_ARG, "negative stride");
  long long full = 0, xc = 0, yc = 0;
  if (__builtin_add_overflow(len, ntaps - 1, &full) || y_off > full || y_len > full - y_off)
    return fail(PDSP_ERR_BAD_ARG, "outputs [%lld, %lld + %lld) beyond the full convolution of %lld samples", y_off, y_off,
                y_len, full);
  if (batch > 1 && y_stride < y_len) return fail(PDSP_ERR_BAD_ARG, "y_stride %lld < y_len %lld", y_stride, y_len);
  if (int rc = row_extents(batch, {{x_stride, len, &xc}, {y_stride, y_len, &yc}})) return rc;
  if (batch == 0 || y_len == 0) return PDSP_OK;
  if (!y || (len > 0 && (!x || !h_re || !h_im))) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  // blocks of a row read input that other blocks overwrite when y shares bytes with x: the result would depend on
  // the order in which workgroups run.  Byte ranges of the whole strided extent, as planes_overlap()
  if (len > 0 && host_ranges_overlap(x, (size_t)xc * sizeof(T), y, (size_t)yc * sizeof(T)))
    return fail(PDSP_ERR_BAD_ARG, "output overlaps input");
  // an even filter runs with one zero tap more (same H): P odd makes hop = N - P + 1 even, the aligned fast path
  const int p = (int)(ntaps % 2 == 1 ? ntaps : ntaps + 1);
  const long long hop = plan->n - (p - 1);
  const long long nblk = (y_len + hop - 1) / hop;
  long long items = 0;
  if (__builtin_mul_overflow(batch, nblk, &items) || items > 0x7fffffffLL)
    return fail(PDSP_ERR_BAD_ARG, "batch too large: %lld rows of %lld blocks", batch, nblk);
  DeviceGuard g(plan->device);
  PDSP_HIP_TRY(g.err);
  if (len == 0) {  // nothing but zero padding: y = 0
    PDSP_HIP_TRY(hipMemset2DAsync(y, (size_t)(batch > 1 ? y_stride : y_len) * sizeof(T), 0, (size_t)y_len * sizeof(T),
                                  (size_t)batch, s));
    return PDSP_OK;
  }
  return fir_filter_dev<T>(plan, batch, x, len, x_stride, h_re, h_im, p, y_off, y_len, y, y_stride, nblk, s);
}

// Block size of the host form (and of FirFilter's default): DESIGN.md, "FIR filtering".
long long fir_block_for(long long ntaps) {
  long long n = 4096;
  while (n < 8 * ntaps && n < 16384) n *= 2;
  while (n / 2 < ntaps) n *= 2;  // never below 2P (the caller has checked ntaps <= 8192)
  return n;
}

}  // namespace pdsp_host

int pdsp_fir_spectrum_f32(const pdsp_plan *plan, const float *taps, long long ntaps, float *h_re, float *h_im,
                          pdsp_stream stream) {
  return fir_spectrum_t<float>(plan, taps, ntaps, h_re, h_im, (hipStream_t)stream);
}
int pdsp_fir_spectrum_f64(const pdsp_plan *plan, const double *taps, long long ntaps, double *h_re, double *h_im,
                          pdsp_stream stream) {
  return fir_spectrum_t<double>(plan, taps, ntaps, h_re, h_im, (hipStream_t)stream);
}
int pdsp_fir_filter_f32(const pdsp_plan *plan, long long batch, const float *x, long long len, long long x_stride,
                        const float *h_re, const float *h_im, long long ntaps, long long y_off, long long y_len, float *y,
                        long long y_stride, pdsp_stream stream) {
  return fir_filter_t<float>(plan, batch, x, len, x_stride, h_re, h_im, ntaps, y_off, y_len, y, y_stride,
                             (hipStream_t)stream);
}
int pdsp_fir_filter_f64(const pdsp_plan *plan, long long batch, const double *x, long long len, long long x_stride,
                        const double *h_re, const double *h_im, long long ntaps, long long y_off, long long y_len,
                        double *y, long long y_stride, pdsp_stream stream) {
  return fir_filter_t<double>(plan, batch, x, len, x_stride, h_re, h_im, ntaps, y_off, y_len, y, y_stride,
                              (hipStream_t)stream);
}

long long pdsp_fir_block_size(long long ntaps) {
  if (ntaps < 1 || ntaps > 8192) return 0;
  return fir_block_for(ntaps);
}

int pdsp_fir_output_range(long long len, long long ntaps, int mode, long long *y_off, long long *y_len) {
  if (len < 1 || ntaps < 1) return fail(PDSP_ERR_BAD_ARG, "signal and filter must not be empty (len %lld, ntaps %lld)", len, ntaps);
  if (!y_off || !y_len) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const long long m = len < ntaps ? len : ntaps;
  switch (mode) {
    case PDSP_FIR_FULL: *y_off = 0, *y_len = len + ntaps - 1; break;
    case PDSP_FIR_SAME: *y_off = (m - 1) / 2, *y_len = len > ntaps ? len : ntaps; break;
    case PDSP_FIR_VALID: *y_off = m - 1, *y_len = (len > ntaps ? len - ntaps : ntaps - len) + 1; break;
    case PDSP_FIR_FILTER: *y_off = 0, *y_len = len; break;
    default: return fail(PDSP_ERR_BAD_ARG, "unknown FIR mode %d", mode);
  }
  return PDSP_OK;
}

int pdsp_fir_filter_host_f64(const double *x, long long batch, long long len, const double *taps, long long ntaps,
                             int mode, double *y) {
  if (batch < 0) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 0, got %lld", batch);
  if (ntaps < 1) return fail(PDSP_ERR_BAD_ARG, "filter must have at least one tap, got %lld", ntaps);
  long long y_off = 0, y_len = 0;
  if (int rc = pdsp_fir_output_range(len, ntaps, mode, &y_off, &y_len)) return rc;
  if (ntaps > 8192)
    return fail(PDSP_ERR_UNSUPPORTED_SIZE, "filter of %lld taps exceeds N/2 = 8192 of the largest block (no partitioned convolution)",
                ntaps);
  long long xs = 0, ys = 0;
  if (!host_count_ok(batch, len, &xs) || !host_count_ok(batch, y_len, &ys))
    return fail(PDSP_ERR_BAD_ARG, "batch %lld x length overflows", batch);
  if (batch == 0) return PDSP_OK;
  if (!x || !taps || !y) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (int rc = require_device()) return rc;
  CachedPlan cp;
  if (int rc = cached_plan(fir_block_for(ntaps), &cp)) return rc;
  const long long bins = cp.plan->n / 2 + 1;
  DeviceBuf sc;
  const size_t nx = (size_t)xs, ny = (size_t)ys, nh = (size_t)(2 * bins);
  PDSP_HIP_TRY(hipMalloc((void **)&sc.d, (nx + ny + nh + (size_t)ntaps) * sizeof(double)));
  double *dx = sc.d, *dy = sc.d + nx, *dh = sc.d + nx + ny, *dt = dh + nh;
  PDSP_HIP_TRY(hipMemcpy(dx, x, nx * sizeof(double), hipMemcpyHostToDevice));
  PDSP_HIP_TRY(hipMemcpy(dt, taps, (size_t)ntaps * sizeof(double), hipMemcpyHostToDevice));
  if (int rc = fir_spectrum_t<double>(cp.plan, dt, ntaps, dh, dh + bins, nullptr)) return rc;
  if (int rc = fir_filter_t<double>(cp.plan, batch, dx, len, len, dh, dh + bins, ntaps, y_off, y_len, dy, y_len, nullptr))
    return rc;
  PDSP_HIP_TRY(hipMemcpy(y, dy, ny * sizeof(double), hipMemcpyDeviceToHost));
  return PDSP_OK;
}

/* ---- short-time transform (complex bins) and its overlap-add inverse -------- */

namespace pdsp_host {

template <typename T>
int stft_complex_t(const pdsp_plan *plan, long long batch, const T *frames, long long frame_len, long long frame_stride,
                   const T *window, T *re_out, T *im_out, hipStream_t s) {
  if (int rc = check_packed_plan<T>(plan, "STFT", false)) return rc;
  if (batch < 1) return fail(PDSP_ERR_BAD_ARG, "frames must be >= 1, got %lld", batch);
  if (frame_len < 1) return fail(PDSP_ERR_BAD_ARG, "frame_len must be >= 1, got %lld", frame_len);
  if (frame_stride < 1) return fail(PDSP_ERR_BAD_ARG, "frame_stride (hop) must be >= 1, got %lld", frame_stride);
  if (batch > 0x7fffffffLL) return fail(PDSP_ERR_BAD_ARG, "batch too large: %lld", batch);
  const long long n = plan->n, bins = n / 2 + 1, used = frame_len < n ? frame_len : n;
  long long in_count = 0, out_count = 0;
  if (int rc = row_extents(batch, {{frame_stride, used, &in_count}, {bins, bins, &out_count}})) return rc;
  if (!frames || !re_out || !im_out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const size_t ib = (size_t)in_count * sizeof(T), ob = (size_t)out_count * sizeof(T), wb = (size_t)n * sizeof(T);
  if (host_ranges_overlap(re_out, ob, frames, ib) || host_ranges_overlap(im_out, ob, frames, ib) ||
      host_ranges_overlap(re_out, ob, im_out, ob) || host_ranges_overlap(re_out, ob, window, wb) ||
      host_ranges_overlap(im_out, ob, window, wb))
    return fail(PDSP_ERR_BAD_ARG, "output overlaps input");
  DeviceGuard g(plan->device);
  PDSP_HIP_TRY(g.err);
  return stft_complex_dev<T>(plan, batch, frames, used, frame_stride, window, re_out, im_out, s);
}

template <typename T>
int istft_t(const pdsp_plan *plan, long long frames, const T *re_in, const T *im_in, long long hop, const T *window, T *out,
            hipStream_t s) {
  if (int rc = check_packed_plan<T>(plan, "STFT", false)) return rc;
  if (frames < 1) return fail(PDSP_ERR_BAD_ARG, "frames must be >= 1, got %lld", frames);
  if (hop < 1) return fail(PDSP_ERR_BAD_ARG, "hop must be >= 1, got %lld", hop);
  if (frames > 0x7fffffffLL) return fail(PDSP_ERR_BAD_ARG, "batch too large: %lld", frames);
  const long long n = plan->n, bins = n / 2 + 1;
  long long total = 0, in_count = 0;
  if (!mad_ok(frames - 1, hop, n, &total) || !mad_ok(frames, bins, 0, &in_count) || total > (LLONG_MAX / 8) ||
      in_count > (LLONG_MAX / 8))
    return fail(PDSP_ERR_BAD_ARG, "frames %lld x hop %lld overflows", frames, hop);
  if (!re_in || !im_in || !out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const size_t ib = (size_t)in_count * sizeof(T), ob = (size_t)total * sizeof(T), wb = (size_t)n * sizeof(T);
  if (host_ranges_overlap(out, ob, re_in, ib) || host_ranges_overlap(out, ob, im_in, ib) ||
      host_ranges_overlap(out, ob, window, wb))
    return fail(PDSP_ERR_BAD_ARG, "output overlaps input");
  DeviceGuard g(plan->device);
  PDSP_HIP_TRY(g.err);
  return istft_dev<T>(plan, frames, re_in, im_in, hop, window, out, s);
}

// Host forms: size, range and window type in the order of the device forms; the plan and its window come from the
// host entry points' plan cache.
int stft_host_checks(long long fft_size, long long hop, int window_type) {
  if (int rc = check_packed_size(fft_size, "STFT")) return rc;
  if (hop < 1) return fail(PDSP_ERR_BAD_ARG, "hop must be >= 1, got %lld", hop);
  if (window_type < PDSP_WIN_RECT || window_type > PDSP_WIN_BLACKMAN)
    return fail(PDSP_ERR_WINDOW_TYPE, "Unsupported window type: %d", window_type);
  return PDSP_OK;
}

}  // namespace pdsp_host

int pdsp_stft_complex_f32(const pdsp_plan *plan, long long batch, const float *frames, long long frame_len,
                          long long frame_stride, const float *window, float *re_out, float *im_out, pdsp_stream stream) {
  return stft_complex_t<float>(plan, batch, frames, frame_len, frame_stride, window, re_out, im_out, (hipStream_t)stream);
}
int pdsp_stft_complex_f64(const pdsp_plan *plan, long long batch, const double *frames, long long frame_len,
                          long long frame_stride, const double *window, double *re_out, double *im_out,
                          pdsp_stream stream) {
  return stft_complex_t<double>(plan, batch, frames, frame_len, frame_stride, window, re_out, im_out, (hipStream_t)stream);
}
int pdsp_istft_f32(const pdsp_plan *plan, long long frames, const float *re_in, const float *im_in, long long hop,
                   const float *window, float *out, pdsp_stream stream) {
  return istft_t<float>(plan, frames, re_in, im_in, hop, window, out, (hipStream_t)stream);
}
int pdsp_istft_f64(const pdsp_plan *plan, long long frames, const double *re_in, const double *im_in, long long hop,
                   const double *window, double *out, pdsp_stream stream) {
  return istft_t<double>(plan, frames, re_in, im_in, hop, window, out, (hipStream_t)stream);
}

int pdsp_set_istft_chunk_frames(int frames) { return std::exchange(g_istft_chunk_frames, frames > 0 ? frames : 0); }

int pdsp_stft_host_f64(const double *signal, long long len, long long fft_size, long long hop, int window_type,
                       double *re_out, double *im_out) {
  if (int rc = stft_host_checks(fft_size, hop, window_type)) return rc;
  if (len < fft_size)
    return fail(PDSP_ERR_INPUT_LENGTH, "signal length %lld is shorter than one frame (%lld)", len, fft_size);
  const long long frames = 1 + (len - fft_size) / hop, bins = fft_size / 2 + 1;
  if (frames > 0x7fffffffLL || len > (1LL << 40)) return fail(PDSP_ERR_BAD_ARG, "signal too long: %lld samples", len);
  if (!signal || !re_out || !im_out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const size_t nx = (size_t)len, ny = (size_t)(frames * bins);  // buffer: signal | re | im
  return packed_host_call(
      fft_size, window_type, nx + 2 * ny,
      [&](pdsp_plan *plan, hipStream_t s, const double *win, double *d) -> int {
        PDSP_HIP_TRY(hipMemcpyAsync(d, signal, nx * sizeof(double), hipMemcpyHostToDevice, s));
        return stft_complex_t<double>(plan, frames, d, fft_size, hop, win, d + nx, d + nx + ny, s);
      },
      [&](const double *d) -> int {
        PDSP_HIP_TRY(hipMemcpy(re_out, d + nx, ny * sizeof(double), hipMemcpyDeviceToHost));
        PDSP_HIP_TRY(hipMemcpy(im_out, d + nx + ny, ny * sizeof(double), hipMemcpyDeviceToHost));
        return PDSP_OK;
      });
}

int pdsp_istft_host_f64(const double *re, const double *im, long long frames, long long fft_size, long long hop,
                        int window_type, double *out) {
  if (int rc = stft_host_checks(fft_size, hop, window_type)) return rc;
  if (frames < 1) return fail(PDSP_ERR_BAD_ARG, "frames must be >= 1, got %lld", frames);
  const long long bins = fft_size / 2 + 1;
  long long total = 0, in_count = 0;
  if (frames > 0x7fffffffLL || !mad_ok(frames - 1, hop, fft_size, &total) || total > (1LL << 40) ||
      !host_count_ok(frames, bins, &in_count))
    return fail(PDSP_ERR_BAD_ARG, "frames %lld x hop %lld overflows", frames, hop);
  if (!re || !im || !out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const size_t nin = (size_t)in_count, ny = (size_t)total;  // buffer: re | im | signal
  return packed_host_call(
      fft_size, window_type, 2 * nin + ny,
      [&](pdsp_plan *plan, hipStream_t s, const double *win, double *d) -> int {
        PDSP_HIP_TRY(hipMemcpyAsync(d, re, nin * sizeof(double), hipMemcpyHostToDevice, s));
        PDSP_HIP_TRY(hipMemcpyAsync(d + nin, im, nin * sizeof(double), hipMemcpyHostToDevice, s));
        return istft_t<double>(plan, frames, d, d + nin, hop, win, d + 2 * nin, s);
      },
      [&](const double *d) -> int {
        PDSP_HIP_TRY(hipMemcpy(out, d + 2 * nin, ny * sizeof(double), hipMemcpyDeviceToHost));
        return PDSP_OK;
      });
}

/* ---- discrete cosine transform, types 2 and 3 ------------------------------ */

namespace pdsp_host {

int check_dct_type_norm(int type, int norm) {
  if (type != 2 && type != 3) return fail(PDSP_ERR_BAD_ARG, "DCT type must be 2 or 3, got %d", type);
  if (norm < PDSP_DCT_BACKWARD || norm > PDSP_DCT_FORWARD)
    return fail(PDSP_ERR_BAD_ARG, "DCT norm must be 0 (backward), 1 (ortho) or 2 (forward), got %d", norm);
  return PDSP_OK;
}

// scipy's norm as the kernels' two scalars, computed in f64 and rounded once: g for every output (type 2) or input
// (type 3), g0 for index 0 instead
void dct_scales(long long n, int type, int norm, double *g, double *g0) {
  const double nn = (double)n;
  if (norm == PDSP_DCT_FORWARD) {
    *g = *g0 = 1.0 / (2.0 * nn);
  } else if (norm == PDSP_DCT_ORTHO) {
    *g = 1.0 / std::sqrt(2.0 * nn);
    *g0 = type == 2 ? 1.0 / std::sqrt(4.0 * nn) : 1.0 / std::sqrt(nn);
  } else {
    *g = *g0 = 1.0;
  }
}

template <typename T>
int dct_t(const pdsp_plan *plan, long long batch, const T *x, long long x_stride, int type, int norm, T *y,
          long long y_stride, hipStream_t s) {
  if (int rc = check_packed_plan<T>(plan, "DCT", true)) return rc;
  const long long n = plan->n;
  if (batch < 1) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 1, got %lld", batch);
  if (x_stride < n || y_stride < n)
    return fail(PDSP_ERR_BAD_ARG, "strides must be >= N = %lld, got x_stride %lld, y_stride %lld", n, x_stride, y_stride);
  if (int rc = check_dct_type_norm(type, norm)) return rc;
  long long xc = 0, yc = 0;
  if (int rc = row_extents(batch, {{x_stride, n, &xc}, {y_stride, n, &yc}})) return rc;
  if (batch > 0x7fffffffLL) return fail(PDSP_ERR_BAD_ARG, "batch too large: %lld", batch);
  if (!x || !y) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  // exact in place is safe (each row is loaded in full by its own workgroup before that workgroup's first barrier);
  // any other overlap would let one row's stores reach another row's loads
  if (!exact_in_place(y, y_stride, x, x_stride) && host_ranges_overlap(y, (size_t)yc * sizeof(T), x, (size_t)xc * sizeof(T)))
    return fail(PDSP_ERR_BAD_ARG, "output overlaps input (only y == x with y_stride == x_stride may share bytes)");
  double g = 1.0, g0 = 1.0;
  dct_scales(n, type, norm, &g, &g0);
  DeviceGuard dg(plan->device);
  PDSP_HIP_TRY(dg.err);
  return dct_dev<T>(plan, batch, x, x_stride, type, (T)g, (T)g0, y, y_stride, s);
}

}  // namespace pdsp_host

int pdsp_dct_f32(const pdsp_plan *plan, long long batch, const float *x, long long x_stride, int type, int norm,
                 float *y, long long y_stride, pdsp_stream stream) {
  return dct_t<float>(plan, batch, x, x_stride, type, norm, y, y_stride, (hipStream_t)stream);
}
int pdsp_dct_f64(const pdsp_plan *plan, long long batch, const double *x, long long x_stride, int type, int norm,
                 double *y, long long y_stride, pdsp_stream stream) {
  return dct_t<double>(plan, batch, x, x_stride, type, norm, y, y_stride, (hipStream_t)stream);
}

int pdsp_dct_host_f64(const double *x, long long batch, long long n, int type, int norm, double *y) {
  if (int rc = check_packed_size(n, "DCT")) return rc;
  if (batch < 1) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 1, got %lld", batch);
  if (int rc = check_dct_type_norm(type, norm)) return rc;
  long long count = 0;
  if (batch > 0x7fffffffLL || !host_count_ok(batch, n, &count))
    return fail(PDSP_ERR_BAD_ARG, "batch %lld x %lld overflows", batch, n);
  if (!x || !y) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const size_t nx = (size_t)count;
  return packed_host_call(
      n, PDSP_WIN_RECT, nx,
      [&](pdsp_plan *plan, hipStream_t s, const double *, double *d) -> int {
        PDSP_HIP_TRY(hipMemcpyAsync(d, x, nx * sizeof(double), hipMemcpyHostToDevice, s));
        return dct_t<double>(plan, batch, d, n, type, norm, d, n, s);  // in place
      },
      [&](const double *d) -> int {
        PDSP_HIP_TRY(hipMemcpy(y, d, nx * sizeof(double), hipMemcpyDeviceToHost));
        return PDSP_OK;
      });
}

/* ---- Hilbert transform, analytic signal, envelope and phase ---------------- */

namespace pdsp_host {

int check_hilbert_mode(int out_mode) {
  if (out_mode < PDSP_HILBERT_ANALYTIC || out_mode > PDSP_HILBERT_PHASE)
    return fail(PDSP_ERR_BAD_ARG, "Hilbert output must be 0 (analytic), 1 (imag), 2 (envelope) or 3 (phase), got %d",
                out_mode);
  return PDSP_OK;
}

template <typename T>
int hilbert_t(const pdsp_plan *plan, long long batch, const T *x, long long x_stride, long long len, int out_mode, T *y,
              long long y_stride, hipStream_t s) {
  if (int rc = check_packed_plan<T>(plan, "the Hilbert transform", false)) return rc;
  const long long n = plan->n;
  if (batch < 1) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 1, got %lld", batch);
  if (len < 1 || len > n) return fail(PDSP_ERR_BAD_ARG, "len must be 1 ... N = %lld, got %lld", n, len);
  if (int rc = check_hilbert_mode(out_mode)) return rc;
  const long long yn = out_mode == PDSP_HILBERT_ANALYTIC ? 2 * n : n;  // values per output row
  if (x_stride < len || y_stride < yn)
    return fail(PDSP_ERR_BAD_ARG, "strides must be >= len = %lld (x) and >= %lld (y), got x_stride %lld, y_stride %lld",
                len, yn, x_stride, y_stride);
  long long xc = 0, yc = 0;
  if (int rc = row_extents(batch, {{x_stride, len, &xc}, {y_stride, yn, &yc}})) return rc;
  if (batch > 0x7fffffffLL) return fail(PDSP_ERR_BAD_ARG, "batch too large: %lld", batch);
  if (!x || !y) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  // exact in place is safe in the N-out modes (a row is loaded in full by its own workgroup before that workgroup's
  // first barrier, and a thread stores only to the samples it has just re-read); any other overlap would let one
  // row's stores reach another row's loads, and ANALYTIC writes two values per sample
  const bool in_place = out_mode != PDSP_HILBERT_ANALYTIC && exact_in_place(y, y_stride, x, x_stride);
  if (!in_place && host_ranges_overlap(y, (size_t)yc * sizeof(T), x, (size_t)xc * sizeof(T)))
    return fail(PDSP_ERR_BAD_ARG, "output overlaps input (only y == x with y_stride == x_stride may share bytes, and "
                                  "not in analytic mode)");
  DeviceGuard dg(plan->device);
  PDSP_HIP_TRY(dg.err);
  return hilbert_dev<T>(plan, batch, x, x_stride, len, out_mode, y, y_stride, s);
}

}  // namespace pdsp_host

int pdsp_hilbert_f32(const pdsp_plan *plan, long long batch, const float *x, long long x_stride, long long len,
                     int out_mode, float *y, long long y_stride, pdsp_stream stream) {
  return hilbert_t<float>(plan, batch, x, x_stride, len, out_mode, y, y_stride, (hipStream_t)stream);
}
int pdsp_hilbert_f64(const pdsp_plan *plan, long long batch, const double *x, long long x_stride, long long len,
                     int out_mode, double *y, long long y_stride, pdsp_stream stream) {
  return hilbert_t<double>(plan, batch, x, x_stride, len, out_mode, y, y_stride, (hipStream_t)stream);
}

int pdsp_hilbert_host_f64(const double *x, long long batch, long long len, long long n, int out_mode, double *y) {
  if (int rc = check_packed_size(n, "the Hilbert transform")) return rc;
  if (batch < 1) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 1, got %lld", batch);
  if (len < 1 || len > n) return fail(PDSP_ERR_BAD_ARG, "len must be 1 ... N = %lld, got %lld", n, len);
  if (int rc = check_hilbert_mode(out_mode)) return rc;
  const long long yn = out_mode == PDSP_HILBERT_ANALYTIC ? 2 * n : n;
  long long xcount = 0, ycount = 0;
  if (batch > 0x7fffffffLL || !host_count_ok(batch, len, &xcount) || !host_count_ok(batch, yn, &ycount))
    return fail(PDSP_ERR_BAD_ARG, "batch %lld x %lld overflows", batch, n);
  if (!x || !y) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  // buffer: y | x, rows of n values on the device whatever len is (the wide path's layout)
  const size_t ny = (size_t)ycount, nx = (size_t)(batch * n);
  return packed_host_call(
      n, PDSP_WIN_RECT, ny + nx,
      [&](pdsp_plan *plan, hipStream_t s, const double *, double *d) -> int {
        PDSP_HIP_TRY(hipMemcpy2DAsync(d + ny, (size_t)n * sizeof(double), x, (size_t)len * sizeof(double),
                                      (size_t)len * sizeof(double), (size_t)batch, hipMemcpyHostToDevice, s));
        return hilbert_t<double>(plan, batch, d + ny, n, len, out_mode, d, yn, s);
      },
      [&](const double *d) -> int {
        PDSP_HIP_TRY(hipMemcpy(y, d, ny * sizeof(double), hipMemcpyDeviceToHost));
        return PDSP_OK;
      });
}

/* ---- polyphase rate change: upfirdn / resample_poly -------------------------- */

// A resampler is its tap table: no FFT size, so no plan.  The table is kept in f64, phase-major
// (g[p][j] = h[p + j up], up rows of T = ceil(ntaps / up), zero-padded), rounded once per precision and uploaded on
// first use (TableHandle, first_use_table).
struct pdsp_resampler : TableHandle {
  long long up = 1, down = 1, ntaps = 1, t0 = 0;
  std::vector<double> taps;  // as convolved (resample_poly: times up)
  std::vector<double> g;
  float *g32 = nullptr;
  double *g64 = nullptr;
  template <typename T>
  auto &slot() {
    if constexpr (sizeof(T) == 4) return g32;
    else return g64;
  }
};

namespace pdsp_host {

constexpr long long kResampleMaxRatio = 8192, kResampleMaxTaps = 8192;

long long gcd_ll(long long a, long long b) {
  while (b) {
    const long long t = a % b;
    a = b, b = t;
  }
  return a;
}

int check_resample_ratio(long long up, long long down) {
  if (up < 1 || down < 1) return fail(PDSP_ERR_BAD_ARG, "up and down must be >= 1, got up %lld, down %lld", up, down);
  if (up > kResampleMaxRatio || down > kResampleMaxRatio)
    return fail(PDSP_ERR_UNSUPPORTED_SIZE, "up and down must be <= %lld, got up %lld, down %lld", kResampleMaxRatio, up,
                down);
  return PDSP_OK;
}

int check_resample_ntaps(long long ntaps) {
  if (ntaps < 1) return fail(PDSP_ERR_BAD_ARG, "filter must have at least one tap, got %lld", ntaps);
  if (ntaps > kResampleMaxTaps)
    return fail(PDSP_ERR_UNSUPPORTED_SIZE, "filter of %lld taps exceeds the %lld a resampler holds", ntaps,
                kResampleMaxTaps);
  return PDSP_OK;
}

// I0(x), the power series sum_k ((x/2)^k / k!)^2, until a term falls below 1e-17 of the sum
double bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-17 * sum) break;
  }
  return sum;
}

// scipy.signal.firwin(2 half + 1, 1 / m, window=("kaiser", 5.0)) * up, half = 10 m, m = max(up, down): a sinc of
// cutoff 1 / m (Nyquist = 1) under a Kaiser window, normalised to unit gain at DC.  up, down already reduced.
void design_taps(long long up, long long down, std::vector<double> *h) {
  const long long m = up > down ? up : down, half = 10 * m, n = 2 * half + 1;
  const double c = 1.0 / (double)m, beta = 5.0, i0b = bessel_i0(beta);
  h->assign((size_t)n, 0.0);
  double sum = 0.0;
  for (long long i = 0; i < n; ++i) {
    const double t = (double)(i - half);
    const double a = M_PI * c * t;
    const double sinc = t == 0.0 ? 1.0 : std::sin(a) / a;
    const double r = t / (double)half;
    const double w = bessel_i0(beta * std::sqrt(1.0 - r * r)) / i0b;
    (*h)[(size_t)i] = c * sinc * w;
    sum += (*h)[(size_t)i];
  }
  for (double &v : *h) v = v / sum * (double)up;
}

int resampler_new(int device, long long up, long long down, std::vector<double> taps, long long t0,
                  pdsp_resampler **out) {
  pdsp_resampler *rs = new (std::nothrow) pdsp_resampler();
  if (!rs) return fail(PDSP_ERR_BAD_ARG, "out of host memory");
  rs->device = device < 0 ? -1 : device;
  rs->up = up, rs->down = down, rs->ntaps = (long long)taps.size(), rs->t0 = t0;
  const long long tn = (rs->ntaps + up - 1) / up;
  rs->g.assign((size_t)(up * tn), 0.0);
  for (long long i = 0; i < rs->ntaps; ++i) rs->g[(size_t)((i % up) * tn + i / up)] = taps[(size_t)i];
  rs->taps = std::move(taps);
  *out = rs;
  return PDSP_OK;
}

// The reduction scipy.signal.resample_poly makes: up, down by their gcd; equal -> the identity (one tap, 1);
// otherwise the given taps, or the default design, times up, and t0 = (ntaps - 1) / 2.
int resample_poly_setup(long long up, long long down, const double *taps, long long ntaps, long long *up_r,
                        long long *down_r, std::vector<double> *h, long long *t0) {
  if (int rc = check_resample_ratio(up, down)) return rc;
  if (taps)
    if (int rc = check_resample_ntaps(ntaps)) return rc;
  const long long gcd = gcd_ll(up, down);
  up /= gcd, down /= gcd;
  *up_r = up, *down_r = down;
  if (up == down) {
    h->assign(1, 1.0);
  } else if (taps) {
    h->assign(taps, taps + ntaps);
    for (double &v : *h) v *= (double)up;
  } else {
    const long long n = 20 * (up > down ? up : down) + 1;
    if (n > kResampleMaxTaps)
      return fail(PDSP_ERR_UNSUPPORTED_SIZE,
                  "the default filter for %lld/%lld has %lld taps, beyond the %lld a resampler holds (pass shorter taps)",
                  up, down, n, kResampleMaxTaps);
    design_taps(up, down, h);
  }
  *t0 = ((long long)h->size() - 1) / 2;
  return PDSP_OK;
}

int resample_len(const pdsp_resampler *rs, long long len, int full, long long *y_len) {
  if (len < 1) return fail(PDSP_ERR_BAD_ARG, "len must be >= 1, got %lld", len);
  long long v = 0;
  if (full ? !mad_ok(len - 1, rs->up, rs->ntaps - 1, &v) : !mad_ok(len, rs->up, rs->down - 1, &v))
    return fail(PDSP_ERR_BAD_ARG, "len %lld x up %lld overflows", len, rs->up);
  *y_len = full ? v / rs->down + 1 : v / rs->down;
  return PDSP_OK;
}

template <typename T>
int upfirdn_t(const pdsp_resampler *crs, long long batch, const T *x, long long len, long long x_stride, T *y,
              long long y_len, long long y_stride, hipStream_t s) {
  if (!crs) return fail(PDSP_ERR_BAD_ARG, "resampler is null");
  pdsp_resampler *const rs = const_cast<pdsp_resampler *>(crs);
  if (batch < 0 || y_len < 0) return fail(PDSP_ERR_BAD_ARG, "negative size (batch %lld, y_len %lld)", batch, y_len);
  if (len < 1) return fail(PDSP_ERR_BAD_ARG, "len must be >= 1, got %lld", len);
  if (x_stride < len || y_stride < y_len)
    return fail(PDSP_ERR_BAD_ARG, "strides must be >= len = %lld (x) and >= y_len = %lld (y), got x_stride %lld, y_stride %lld",
                len, y_len, x_stride, y_stride);
  long long xc = 0, yc = 0, q = 0;
  if (int rc = row_extents(batch, {{x_stride, len, &xc}, {y_stride, y_len, &yc}})) return rc;
  if (!mad_ok(y_len, rs->down, rs->t0 + rs->up * rs->down, &q))
    return fail(PDSP_ERR_BAD_ARG, "y_len %lld x down %lld overflows", y_len, rs->down);
  if (batch == 0 || y_len == 0) return PDSP_OK;
  if (!x || !y) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  // a tile reads samples that other tiles' outputs would overwrite: byte ranges of the whole strided extents
  if (host_ranges_overlap(x, (size_t)xc * sizeof(T), y, (size_t)yc * sizeof(T)))
    return fail(PDSP_ERR_BAD_ARG, "output overlaps input");
  if (int rc = require_device()) return rc;
  T *&g = rs->slot<T>();
  if (int rc = first_use_table(*rs, g, s, "tap table", [&] { return std::vector<T>(rs->g.begin(), rs->g.end()); }))
    return rc;
  DeviceGuard dg(rs->device);
  PDSP_HIP_TRY(dg.err);
  return upfirdn_dev<T>(g, rs->up, rs->down, rs->ntaps, rs->t0, batch, x, len, x_stride, y, y_len, y_stride, s);
}

// The host forms: one resampler, one device buffer x | y, the f64 kernel on the null stream (pdsp_fir_filter_host_f64's
// shape: f64 arithmetic whatever pdsp_set_host_precision says).
int resample_host(pdsp_resampler *rs, const double *x, long long batch, long long len, int full, double *y) {
  const HandleOwner<pdsp_resampler> own(rs);
  if (batch < 0) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 0, got %lld", batch);
  long long y_len = 0, xs = 0, ys = 0;
  if (int rc = resample_len(rs, len, full, &y_len)) return rc;
  if (!host_count_ok(batch, len, &xs) || !host_count_ok(batch, y_len, &ys))
    return fail(PDSP_ERR_BAD_ARG, "batch %lld x length overflows", batch);
  if (batch == 0) return PDSP_OK;
  if (!x || !y) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (int rc = require_device()) return rc;
  DeviceBuf sc;
  const size_t nx = (size_t)xs, ny = (size_t)ys;
  PDSP_HIP_TRY(hipMalloc((void **)&sc.d, (nx + ny) * sizeof(double)));
  PDSP_HIP_TRY(hipMemcpy(sc.d, x, nx * sizeof(double), hipMemcpyHostToDevice));
  if (int rc = upfirdn_t<double>(rs, batch, sc.d, len, len, sc.d + nx, y_len, y_len, nullptr)) return rc;
  PDSP_HIP_TRY(hipMemcpy(y, sc.d + nx, ny * sizeof(double), hipMemcpyDeviceToHost));
  return PDSP_OK;
}

}  // namespace pdsp_host

int pdsp_resampler_create(int device, long long up, long long down, const double *taps, long long ntaps, long long t0,
                          pdsp_resampler **out) {
  if (!out) return fail(PDSP_ERR_BAD_ARG, "out is null");
  *out = nullptr;
  if (int rc = check_resample_ratio(up, down)) return rc;
  if (int rc = check_resample_ntaps(ntaps)) return rc;
  if (!taps) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (t0 < 0 || t0 >= ntaps + up)
    return fail(PDSP_ERR_BAD_ARG, "t0 must be 0 ... ntaps + up - 1 = %lld, got %lld", ntaps + up - 1, t0);
  return resampler_new(device, up, down, std::vector<double>(taps, taps + ntaps), t0, out);
}

int pdsp_resampler_create_poly(int device, long long up, long long down, const double *taps_or_null, long long ntaps,
                               pdsp_resampler **out) {
  if (!out) return fail(PDSP_ERR_BAD_ARG, "out is null");
  *out = nullptr;
  std::vector<double> h;
  long long t0 = 0;
  if (int rc = resample_poly_setup(up, down, taps_or_null, ntaps, &up, &down, &h, &t0)) return rc;
  return resampler_new(device, up, down, std::move(h), t0, out);
}

int pdsp_resampler_destroy(pdsp_resampler *rs) { return destroy_handle(rs); }

long long pdsp_resampler_up(const pdsp_resampler *rs) { return rs ? rs->up : 0; }
long long pdsp_resampler_down(const pdsp_resampler *rs) { return rs ? rs->down : 0; }
long long pdsp_resampler_ntaps(const pdsp_resampler *rs) { return rs ? rs->ntaps : 0; }
long long pdsp_resampler_t0(const pdsp_resampler *rs) { return rs ? rs->t0 : 0; }
int pdsp_resampler_taps(const pdsp_resampler *rs, double *taps) {
  if (!rs || !taps) return fail(PDSP_ERR_BAD_ARG, rs ? "null buffer" : "resampler is null");
  std::memcpy(taps, rs->taps.data(), rs->taps.size() * sizeof(double));
  return PDSP_OK;
}

int pdsp_resample_output_len(const pdsp_resampler *rs, long long len, int full, long long *y_len) {
  if (!rs) return fail(PDSP_ERR_BAD_ARG, "resampler is null");
  if (!y_len) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  return resample_len(rs, len, full, y_len);
}

int pdsp_upfirdn_f32(const pdsp_resampler *rs, long long batch, const float *x, long long len, long long x_stride,
                     float *y, long long y_len, long long y_stride, pdsp_stream stream) {
  return upfirdn_t<float>(rs, batch, x, len, x_stride, y, y_len, y_stride, (hipStream_t)stream);
}
int pdsp_upfirdn_f64(const pdsp_resampler *rs, long long batch, const double *x, long long len, long long x_stride,
                     double *y, long long y_len, long long y_stride, pdsp_stream stream) {
  return upfirdn_t<double>(rs, batch, x, len, x_stride, y, y_len, y_stride, (hipStream_t)stream);
}

int pdsp_set_upfirdn_tile(int mode) {
  const int prev = g_upfirdn_tile;
  if (mode >= 0 && (mode & 15) <= 4) g_upfirdn_tile = mode;
  return prev;
}

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

// The host calls' own rule (transform_cut / spectrum_cut) in the precision the call would run in
static int host_cut_out(const pdsp_plan *plan, long long batch, int precision, long long info[2], long long bins) {
  if (int rc = check_plan_batch(plan, batch)) return rc;
  if (!info) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (precision != 32 && precision != 64) return fail(PDSP_ERR_BAD_ARG, "precision must be 32 or 64, got %d", precision);
  const bool f64 = precision == 64 && (plan->t64.tw || (bins && plan->t64.tw_half));
  HostCut c;
  if (batch > 0) {
    if (bins) c = f64 ? spectrum_cut<double>(plan, batch, bins) : spectrum_cut<float>(plan, batch, bins);
    else c = f64 ? transform_cut<double>(plan, batch) : transform_cut<float>(plan, batch);
  }
  const long long nchunks = c.chunked ? (batch + c.per_chunk - 1) / c.per_chunk : 0;
  info[0] = c.chunked ? c.per_chunk : 0;
  info[1] = c.chunked ? (c.workers < nchunks ? c.workers : nchunks) : 0;
  return PDSP_OK;
}
int pdsp_dev_host_transform_chunks(const pdsp_plan *plan, long long batch, int precision, long long info[2]) {
  return host_cut_out(plan, batch, precision, info, 0);
}
int pdsp_dev_host_spectrum_chunks(const pdsp_plan *plan, long long batch, int sides, int precision, long long info[2]) {
  if (sides != PDSP_SIDES_ONE && sides != PDSP_SIDES_TWO) return fail(PDSP_ERR_BAD_ARG, "bad sides %d", sides);
  if (!plan) return fail(PDSP_ERR_BAD_ARG, "plan is null");
  return host_cut_out(plan, batch, precision, info, sides == PDSP_SIDES_ONE ? plan->n / 2 + 1 : plan->n);
}

int pdsp_dev_upfirdn_tile(long long up, long long down, long long ntaps, long long y_len, int elem_bytes,
                          long long info[9]) {
  if (!info) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (int rc = check_resample_ratio(up, down)) return rc;
  if (int rc = check_resample_ntaps(ntaps)) return rc;
  if (y_len < 1) return fail(PDSP_ERR_BAD_ARG, "y_len must be >= 1, got %lld", y_len);
  if (elem_bytes != 4 && elem_bytes != 8) return fail(PDSP_ERR_BAD_ARG, "elem_bytes must be 4 or 8, got %d", elem_bytes);
  UpfirdnTile t;
  if (int rc = upfirdn_tile_checked(up, down, ntaps, y_len, (size_t)elem_bytes, &t)) return rc;
  const long long v[9] = {t.r, t.win, t.gt, t.tn, t.tp, t.bper, t.span, (long long)t.lds_bytes, t.items};
  std::memcpy(info, v, sizeof(v));
  return PDSP_OK;
}

int pdsp_resample_design_f64(long long up, long long down, double *taps, long long *ntaps) {
  if (!ntaps) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  std::vector<double> h;
  long long t0 = 0;
  if (int rc = resample_poly_setup(up, down, nullptr, 0, &up, &down, &h, &t0)) return rc;
  *ntaps = (long long)h.size();
  if (taps) std::memcpy(taps, h.data(), h.size() * sizeof(double));
  return PDSP_OK;
}

int pdsp_resample_poly_host_f64(const double *x, long long batch, long long len, long long up, long long down,
                                const double *taps_or_null, long long ntaps, double *y) {
  pdsp_resampler *rs = nullptr;
  if (int rc = pdsp_resampler_create_poly(-1, up, down, taps_or_null, ntaps, &rs)) return rc;
  return resample_host(rs, x, batch, len, 0, y);
}

int pdsp_upfirdn_host_f64(const double *h, long long ntaps, const double *x, long long batch, long long len,
                          long long up, long long down, double *y) {
  pdsp_resampler *rs = nullptr;
  if (int rc = pdsp_resampler_create(-1, up, down, h, ntaps, 0, &rs)) return rc;
  return resample_host(rs, x, batch, len, 1, y);
}

/* ---- chirp-z rows: the chirp-z transform, the zoom FFT and the any-length DFT ---- */

namespace pdsp_host {

// A chirp-z transform of L samples into K bins is its three tables -- pre[n] = a^-n w^(n^2/2), post[k] = w^(k^2/2) and
// Bt = FFT_M(b) / M of the chirp filter b[j] = w^(-j^2/2) -- evaluated on the host and rounded once per precision, plus
// the radix table of the M-point transform (the tw_half of a plan of 2M points).  They go up at create time through the
// plans' uploader into the handle's own lists (TableHandle).  A DFT is the transform with K = L whose post is its pre,
// the chirp c[n] = exp(-i pi n^2 / L), uploaded once.
template <typename T>
struct ChirpSet {
  typename pdsp::vec2<T>::type *tw = nullptr;  // the M-point radix table
  typename pdsp::vec2<T>::type *pre = nullptr, *post = nullptr, *bt = nullptr;
};
struct ChirpTables : TableHandle {
  long long length = 0, bins = 0, m = 0;
  int log2m = 0;
  ChirpSet<float> s32;
  ChirpSet<double> s64;
  template <typename T>
  const ChirpSet<T> &slot() const {
    if constexpr (sizeof(T) == 4) return s32;
    else return s64;
  }
};

}  // namespace pdsp_host

struct pdsp_dft : pdsp_host::ChirpTables {};
struct pdsp_czt : pdsp_host::ChirpTables {};

namespace pdsp_host {

constexpr long long kDftMinLength = 2, kDftMaxLength = 4096, kCztMaxConv = 8192;
constexpr long double kPiL = 3.141592653589793238462643383279502884L;

// M = max(32, the smallest power of two >= L + K - 1; the DFT's K is L): the circular convolution must hold the
// L + K - 1 lags -(L - 1) ... K - 1 of the chirp filter; 32 is the smallest row of the sixteen-points-per-thread layout
int chirp_log2m(long long length, long long bins) {
  const int l = ilog2ll(length + bins - 1);
  return l < 5 ? 5 : l;
}

// FFT_M(re + i im) / M, rounded to f64.  Radix-2 decimation in time in long double, every twiddle evaluated directly
// (no recurrence): built once per object, M <= 8192.
std::vector<double2> chirp_fft_over_m(std::vector<long double> re, std::vector<long double> im, int log2m) {
  const size_t m = (size_t)1 << log2m;
  for (size_t i = 0; i < m; ++i) {
    size_t r = 0;
    for (int b = 0; b < log2m; ++b) r |= ((i >> b) & 1) << (log2m - 1 - b);
    if (i < r) std::swap(re[i], re[r]), std::swap(im[i], im[r]);
  }
  for (size_t half = 1; half < m; half <<= 1) {
    for (size_t k = 0; k < half; ++k) {
      const long double a = -kPiL * (long double)k / (long double)half;
      const long double wr = cosl(a), wi = sinl(a);
      for (size_t i = k; i < m; i += 2 * half) {
        const size_t j = i + half;
        const long double tr = re[j] * wr - im[j] * wi, ti = re[j] * wi + im[j] * wr;
        re[j] = re[i] - tr, im[j] = im[i] - ti;
        re[i] += tr, im[i] += ti;
      }
    }
  }
  std::vector<double2> bt(m);
  for (size_t k = 0; k < m; ++k) bt[k] = double2{(double)(re[k] / (long double)m), (double)(im[k] / (long double)m)};
  return bt;
}

template <typename T2>
std::vector<T2> chirp_round(const std::vector<double2> &v) {
  std::vector<T2> r(v.size());
  for (size_t i = 0; i < v.size(); ++i) r[i].x = (decltype(r[i].x))v[i].x, r[i].y = (decltype(r[i].y))v[i].y;
  return r;
}

// The object of one transform on `device` (< 0: the current one), behind its creator's own argument checks: its
// tables in both precisions.  post null: the DFT, whose post is its pre.  what: the transform's name in the message.
template <class H>
int chirp_create(H **out, const char *what, int device, long long length, long long bins,
                 const std::vector<double2> &pre, const std::vector<double2> *post, const std::vector<double2> &bt) {
  if (int rc = require_device()) return rc;
  if (int rc = resolve_device(&device)) return rc;
  DeviceGuard g(device);
  PDSP_HIP_TRY(g.err);
  H *h = new (std::nothrow) H();
  if (!h) return fail(PDSP_ERR_BAD_ARG, "out of host memory");
  h->device = device, h->length = length, h->bins = bins, h->log2m = chirp_log2m(length, bins), h->m = 1LL << h->log2m;
  auto upload = [&](auto &t, auto &s) -> hipError_t {
    using T2 = std::remove_pointer_t<decltype(s.pre)>;
    if (hipError_t e = upload_table(t, build_twiddles<T2>(h->log2m), &s.tw)) return e;
    if (hipError_t e = upload_table(t, chirp_round<T2>(pre), &s.pre)) return e;
    if (!post) s.post = s.pre;
    else if (hipError_t e = upload_table(t, chirp_round<T2>(*post), &s.post)) return e;
    return upload_table(t, chirp_round<T2>(bt), &s.bt);
  };
  hipError_t e = upload(h->t32, h->s32);
  if (e == hipSuccess) e = upload(h->t64, h->s64);
  if (e != hipSuccess) {
    destroy_handle(h);
    return fail(PDSP_ERR_DEVICE, "HIP error %d (%s) at hipMalloc / hipMemcpy of the %s tables", (int)e,
                hipGetErrorString(e), what);
  }
  *out = h;
  return PDSP_OK;
}

// The row arguments of one launch, then the launch.  dft: 0 the chirp-z transform (czt_dev), +1 / -1 the forward /
// inverse DFT (dft_dev).  Exact in place is safe: a workgroup loads all of its rows in full before its first barrier and stores
// only into those rows, and with equal strides >= max(L, K) a row's samples and its bins share one slot that no other
// row touches.  Any other overlap would let one row's stores reach another row's loads, or one plane's stores the other
// plane's loads of the same row.  The two transforms keep their own in-place rules.  The chirp-z transform takes a real
// row in place as well, its im_out apart, and compares the two planes over the larger of the two extents: the samples
// of the last row may reach past its bins.  The DFT takes complex rows only: a real row has no in-place form, and with
// K = L the output-plane check is the whole comparison.
template <typename T>
int chirp_t(const ChirpTables &c, int dft, long long batch, const T *re_in, const T *im_in, long long in_stride,
            T *re_out, T *im_out, long long out_stride, hipStream_t s) {
  const long long n = c.length, k = c.bins;
  if (batch < 1) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 1, got %lld", batch);
  if (in_stride < n || out_stride < k)
    return fail(PDSP_ERR_BAD_ARG, "strides must be >= L = %lld in and >= K = %lld out, got in_stride %lld, out_stride %lld",
                n, k, in_stride, out_stride);
  long long ic = 0, oc = 0;
  if (int rc = row_extents(batch, {{in_stride, n, &ic}, {out_stride, k, &oc}})) return rc;
  if (batch > 0x7fffffffLL) return fail(PDSP_ERR_BAD_ARG, "batch too large: %lld", batch);
  if (!re_in || !re_out || !im_out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const size_t ib = (size_t)ic * sizeof(T), ob = (size_t)oc * sizeof(T), xb = ib > ob ? ib : ob;
  const bool in_place = exact_in_place(re_out, out_stride, re_in, in_stride) &&
                        (im_in ? (const void *)im_out == (const void *)im_in : !dft);
  const bool clash = !in_place ? (host_ranges_overlap(re_out, ob, re_in, ib) || host_ranges_overlap(re_out, ob, im_in, ib) ||
                                  host_ranges_overlap(im_out, ob, re_in, ib) || host_ranges_overlap(im_out, ob, im_in, ib))
                     : dft     ? false
                     : im_in   ? host_ranges_overlap(re_in, xb, im_in, xb)
                               : host_ranges_overlap(im_out, ob, re_in, xb);
  if (clash)
    return fail(PDSP_ERR_BAD_ARG, "output overlaps input (only re_out == re_in, im_out == im_in%s with equal strides "
                                  "may share bytes)", dft ? "" : " -- a real row's im_out apart --");
  if (host_ranges_overlap(re_out, ob, im_out, ob))
    return fail(PDSP_ERR_BAD_ARG, "the output planes overlap each other");
  const ChirpSet<T> &v = c.slot<T>();
  DeviceGuard dg(c.device);
  PDSP_HIP_TRY(dg.err);
  if (dft)
    return dft_dev<T>(c.log2m, n, batch, re_in, im_in, in_stride, re_out, im_out, out_stride, v.pre, v.bt, v.tw,
                      dft < 0, s);
  return czt_dev<T>(c.log2m, n, k, batch, re_in, im_in, in_stride, re_out, im_out, out_stride, v.pre, v.post, v.bt, v.tw,
                    s);
}

// The host forms ride the packed features' scaffold on the cached plan of 2M points (64 ... 16384: its stream, its
// lock, its device), behind their own size checks; the transform's own tables live for the call: create(device, &h).
// Buffer: out re | out im | in re | in im.
template <class H, class Create>
int chirp_host(int dft, const double *re_in, const double *im_in, long long batch, long long length, long long bins,
               double *re_out, double *im_out, Create create) {
  if (batch < 1) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 1, got %lld", batch);
  long long cin = 0, cout = 0;
  if (batch > 0x7fffffffLL || !host_count_ok(batch, length, &cin) || !host_count_ok(batch, bins, &cout))
    return fail(PDSP_ERR_BAD_ARG, "batch %lld x (%lld, %lld) overflows", batch, length, bins);
  if (!re_in || !re_out || !im_out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const size_t nx = (size_t)cin, ny = (size_t)cout;
  HandleOwner<H> own;
  return packed_host_call(
      2LL << chirp_log2m(length, bins), PDSP_WIN_RECT, 2 * ny + 2 * nx,
      [&](pdsp_plan *plan, hipStream_t s, const double *, double *d) -> int {
        H *h = nullptr;
        if (int rc = create(plan->device, &h)) return rc;
        own.reset(h);
        double *const xr = d + 2 * ny, *const xi = xr + nx;
        PDSP_HIP_TRY(hipMemcpyAsync(xr, re_in, nx * sizeof(double), hipMemcpyHostToDevice, s));
        if (im_in) PDSP_HIP_TRY(hipMemcpyAsync(xi, im_in, nx * sizeof(double), hipMemcpyHostToDevice, s));
        return chirp_t<double>(*own, dft, batch, xr, im_in ? xi : nullptr, length, d, d + ny, bins, s);
      },
      [&](const double *d) -> int {
        PDSP_HIP_TRY(hipMemcpy(re_out, d, ny * sizeof(double), hipMemcpyDeviceToHost));
        PDSP_HIP_TRY(hipMemcpy(im_out, d + ny, ny * sizeof(double), hipMemcpyDeviceToHost));
        return PDSP_OK;
      });
}

/* the any-length DFT: Bluestein's algorithm */

int check_dft_length(long long length) {
  if (length < kDftMinLength || length > kDftMaxLength)
    return fail(PDSP_ERR_UNSUPPORTED_SIZE, "DFT length must be %lld ... %lld, got %lld", kDftMinLength, kDftMaxLength,
                length);
  return PDSP_OK;
}

// c[n] = exp(-i pi n^2 / L), n < L, in f64: the angle's numerator n^2 is reduced mod 2L in integers, so the argument of
// cos / sin stays below 2 pi and carries no rounding of n^2
std::vector<double2> dft_chirp(long long length) {
  std::vector<double2> c((size_t)length);
  for (long long n = 0; n < length; ++n) {
    const double a = -M_PI * (double)((n * n) % (2 * length)) / (double)length;
    c[(size_t)n] = double2{std::cos(a), std::sin(a)};
  }
  return c;
}

// Bt of the even filter b[j] = conj c[|j|] at j and M - j for |j| < L, else 0
std::vector<double2> dft_filter_spectrum(const std::vector<double2> &c, int log2m) {
  const size_t m = (size_t)1 << log2m;
  std::vector<long double> re(m, 0.0L), im(m, 0.0L);
  for (size_t j = 0; j < c.size(); ++j) {
    re[j] = c[j].x, im[j] = -c[j].y;
    if (j) re[m - j] = c[j].x, im[m - j] = -c[j].y;
  }
  return chirp_fft_over_m(std::move(re), std::move(im), log2m);
}

template <typename T>
int dft_t(const pdsp_dft *d, long long batch, const T *re_in, const T *im_in, long long in_stride, T *re_out, T *im_out,
          long long out_stride, int inverse, hipStream_t s) {
  if (!d) return fail(PDSP_ERR_BAD_ARG, "dft is null");
  return chirp_t<T>(*d, inverse ? -1 : 1, batch, re_in, im_in, in_stride, re_out, im_out, out_stride, s);
}

/* the chirp-z transform and zoom FFT */

int check_czt_args(long long length, long long bins, double step, double start, double radius) {
  if (length < 1) return fail(PDSP_ERR_UNSUPPORTED_SIZE, "CZT length must be >= 1, got %lld", length);
  if (bins < 1) return fail(PDSP_ERR_UNSUPPORTED_SIZE, "CZT bins must be >= 1, got %lld", bins);
  if (length > kCztMaxConv || bins > kCztMaxConv || length + bins - 1 > kCztMaxConv)
    return fail(PDSP_ERR_UNSUPPORTED_SIZE, "CZT length + bins - 1 must be <= %lld, got %lld + %lld - 1", kCztMaxConv,
                length, bins);
  // (a double of 2^53 or more is a whole number of turns, or of half turns)
  if (!(std::fabs(step) < 0x1p53) || !(std::fabs(start) < 0x1p53))
    return fail(PDSP_ERR_BAD_ARG, "CZT step and start must be finite numbers of turns below 2^53, got %g and %g", step,
                start);
  if (!(radius > 0.0) || !std::isfinite(radius))
    return fail(PDSP_ERR_BAD_ARG, "CZT radius must be finite and > 0, got %g", radius);
  if (std::fabs((long double)(length - 1) * log2l((long double)radius)) > 64.0L)
    return fail(PDSP_ERR_BAD_ARG, "CZT radius^-(L-1) must lie within [2^-64, 2^64], got radius %.17g at L = %lld",
                radius, length);
  return PDSP_OK;
}

// The tables are evaluated in long double from exactly reduced phases.  (n t) mod `mod` in turns, exactly: n an integer
// below 2^27 (or its square), t the caller's double.  p + e is the product without error; fmod of p is exact; the error
// term is added after the reduction, so the sum carries the product's low bits however large n t is.
long double czt_turns(long long n, double t, double mod) {
  const double p = (double)n * t, e = std::fma((double)n, t, -p);
  return (long double)std::fmod(p, mod) + (long double)e;
}

struct ldcx {
  long double x, y;
};

// w^(sgn n^2 / 2), w = exp(-2 pi i step): the half-turn chirp, n^2 step reduced mod 2
ldcx czt_chirp(long long n, double step, int sgn) {
  const long double a = -(long double)sgn * kPiL * czt_turns(n * n, step, 2.0);
  return ldcx{cosl(a), sinl(a)};
}

template <class F>
std::vector<double2> czt_table(long long count, F f) {
  std::vector<double2> t((size_t)count);
  for (long long i = 0; i < count; ++i) {
    const ldcx v = f(i);
    t[(size_t)i] = double2{(double)v.x, (double)v.y};
  }
  return t;
}

// pre[n] = a^-n w^(n^2/2), a = radius exp(2 pi i start): n start reduced mod 1
std::vector<double2> czt_pre(long long length, double step, double start, double radius) {
  return czt_table(length, [&](long long n) {
    const ldcx c = czt_chirp(n, step, 1);
    const long double a = -2.0L * kPiL * czt_turns(n, start, 1.0), r = powl((long double)radius, -(long double)n);
    const long double ar = r * cosl(a), ai = r * sinl(a);
    return ldcx{ar * c.x - ai * c.y, ar * c.y + ai * c.x};
  });
}

std::vector<double2> czt_post(long long bins, double step) {
  return czt_table(bins, [&](long long k) { return czt_chirp(k, step, 1); });
}

// Bt of b[j] = w^(-j^2/2) at j for 0 <= j < K, at M + j for -(L - 1) <= j < 0, else 0 (M >= L + K - 1: the two runs do
// not meet).  b's support is not symmetric: this is not the DFT's even filter.
std::vector<double2> czt_filter_spectrum(long long length, long long bins, double step, int log2m) {
  const size_t m = (size_t)1 << log2m;
  std::vector<long double> re(m, 0.0L), im(m, 0.0L);
  for (long long j = -(length - 1); j < bins; ++j) {
    const ldcx v = czt_chirp(j, step, -1);
    const size_t at = (size_t)(j < 0 ? (long long)m + j : j);
    re[at] = v.x, im[at] = v.y;
  }
  return chirp_fft_over_m(std::move(re), std::move(im), log2m);
}

template <typename T>
int czt_t(const pdsp_czt *c, long long batch, const T *re_in, const T *im_in, long long in_stride, T *re_out, T *im_out,
          long long out_stride, hipStream_t s) {
  if (!c) return fail(PDSP_ERR_BAD_ARG, "czt is null");
  return chirp_t<T>(*c, 0, batch, re_in, im_in, in_stride, re_out, im_out, out_stride, s);
}

}  // namespace pdsp_host

int pdsp_dft_create(long long length, int device, pdsp_dft **out) {
  if (!out) return fail(PDSP_ERR_BAD_ARG, "out is null");
  if (int rc = check_dft_length(length)) return rc;
  const std::vector<double2> c = dft_chirp(length);
  return chirp_create(out, "DFT", device, length, length, c, nullptr,
                      dft_filter_spectrum(c, chirp_log2m(length, length)));
}

int pdsp_dft_destroy(pdsp_dft *d) { return destroy_handle(d); }
long long pdsp_dft_length(const pdsp_dft *d) { return d ? d->length : 0; }
long long pdsp_dft_conv_size(const pdsp_dft *d) { return d ? d->m : 0; }

int pdsp_dft_c2c_f32(const pdsp_dft *d, long long batch, const float *re_in, const float *im_in, long long in_stride,
                     float *re_out, float *im_out, long long out_stride, int inverse, pdsp_stream stream) {
  return dft_t<float>(d, batch, re_in, im_in, in_stride, re_out, im_out, out_stride, inverse, (hipStream_t)stream);
}
int pdsp_dft_c2c_f64(const pdsp_dft *d, long long batch, const double *re_in, const double *im_in, long long in_stride,
                     double *re_out, double *im_out, long long out_stride, int inverse, pdsp_stream stream) {
  return dft_t<double>(d, batch, re_in, im_in, in_stride, re_out, im_out, out_stride, inverse, (hipStream_t)stream);
}

int pdsp_dft_host_f64(const double *re_in, const double *im_in, long long batch, long long length, int inverse,
                      double *re_out, double *im_out) {
  if (int rc = check_dft_length(length)) return rc;
  return chirp_host<pdsp_dft>(inverse ? -1 : 1, re_in, im_in, batch, length, length, re_out, im_out,
                              [&](int device, pdsp_dft **d) { return pdsp_dft_create(length, device, d); });
}

int pdsp_czt_create(long long length, long long bins, double step, double start, double radius, int device,
                    pdsp_czt **out) {
  if (!out) return fail(PDSP_ERR_BAD_ARG, "out is null");
  if (int rc = check_czt_args(length, bins, step, start, radius)) return rc;
  const std::vector<double2> post = czt_post(bins, step);
  return chirp_create(out, "CZT", device, length, bins, czt_pre(length, step, start, radius), &post,
                      czt_filter_spectrum(length, bins, step, chirp_log2m(length, bins)));
}

int pdsp_czt_destroy(pdsp_czt *c) { return destroy_handle(c); }
long long pdsp_czt_length(const pdsp_czt *c) { return c ? c->length : 0; }
long long pdsp_czt_bins(const pdsp_czt *c) { return c ? c->bins : 0; }
long long pdsp_czt_conv_size(const pdsp_czt *c) { return c ? c->m : 0; }

int pdsp_czt_f32(const pdsp_czt *c, long long batch, const float *re_in, const float *im_in, long long in_stride,
                 float *re_out, float *im_out, long long out_stride, pdsp_stream stream) {
  return czt_t<float>(c, batch, re_in, im_in, in_stride, re_out, im_out, out_stride, (hipStream_t)stream);
}
int pdsp_czt_f64(const pdsp_czt *c, long long batch, const double *re_in, const double *im_in, long long in_stride,
                 double *re_out, double *im_out, long long out_stride, pdsp_stream stream) {
  return czt_t<double>(c, batch, re_in, im_in, in_stride, re_out, im_out, out_stride, (hipStream_t)stream);
}

int pdsp_czt_host_f64(const double *re_in, const double *im_in, long long batch, long long length, long long bins,
                      double step, double start, double radius, double *re_out, double *im_out) {
  if (int rc = check_czt_args(length, bins, step, start, radius)) return rc;
  return chirp_host<pdsp_czt>(0, re_in, im_in, batch, length, bins, re_out, im_out, [&](int device, pdsp_czt **c) {
    return pdsp_czt_create(length, bins, step, start, radius, device, c);
  });
}

/* ---- multi-level wavelet transform: wavedec / waverec -------------------------- */

// A wavelet transform is its scaling filter and its depth: no FFT size, so no plan.  The taps are kept in f64, h | g,
// rounded once per precision and uploaded on first use (TableHandle, first_use_table).
struct pdsp_dwt : TableHandle {
  int levels = 1;
  std::vector<double> hg;  // h | g, g[j] = (-1)^j h[F - 1 - j]
  float *hg32 = nullptr;
  double *hg64 = nullptr;
  template <typename T>
  auto &slot() {
    if constexpr (sizeof(T) == 4) return hg32;
    else return hg64;
  }
};

namespace pdsp_host {

constexpr long long kDwtMaxTaps = 32;
constexpr int kDaubechiesMax = 10;
// Daubechies' extremal-phase scaling filters db1 ... db10, sum sqrt 2 (tools/gen_daubechies.py prints this table)
const double kDaubechies[] = {
    // db1
    0.7071067811865476, 0.7071067811865476,
    // db2
    0.48296291314453427, 0.836516303737808, 0.22414386804201333, -0.12940952255126045,
    // db3
    0.3326705529500826, 0.8068915093110924, 0.4598775021184915, -0.1350110200102546,
    -0.08544127388202662, 0.035226291885709554,
    // db4
    0.23037781330889645, 0.7148465705529156, 0.630880767929859, -0.02798376941685959,
    -0.18703481171909309, 0.03084138183556063, 0.03288301166688517, -0.010597401785069018,
    // db5
    0.16010239797419293, 0.6038292697971896, 0.724308528437773, 0.13842814590132088,
    -0.242294887066382, -0.03224486958463847, 0.0775714938400457, -0.006241490212798271,
    -0.012580751999081994, 0.003335725285473771,
    // db6
    0.1115407433501094, 0.4946238903984529, 0.7511339080210949, 0.315250351709198,
    -0.2262646939654393, -0.12976686756726188, 0.09750160558732306, 0.027522865530305606,
    -0.03158203931748598, 0.0005538422011615001, 0.0047772575109455056, -0.0010773010853084794,
    // db7
    0.07785205408500923, 0.3965393194819175, 0.7291320908462354, 0.46978228740519296,
    -0.14390600392856523, -0.22403618499387515, 0.07130921926683047, 0.08061260915108304,
    -0.03802993693501441, -0.016574541630666902, 0.012550998556099856, 0.00042957797292136684,
    -0.0018016407040474935, 0.0003537137999745206,
    // db8
    0.05441584224310395, 0.3128715909142996, 0.6756307362972892, 0.5853546836542065,
    -0.015829105256348515, -0.2840155429615464, 0.00047248457391308016, 0.12874742662047872,
    -0.01736930100180785, -0.04408825393079459, 0.013981027917398262, 0.008746094047405749,
    -0.004870352993451561, -0.0003917403733769474, 0.0006754494064505685, -0.00011747678412476935,
    // db9
    0.03807794736387834, 0.24383467461259023, 0.6048231236901112, 0.6572880780513,
    0.13319738582500756, -0.2932737832791743, -0.096840783222976, 0.14854074933810588,
    0.03072568147933388, -0.06763282906133072, 0.000250947114831909, 0.02236166212367897,
    -0.004723204757751389, -0.004281503682463433, 0.0018476468830562285, 0.00023038576352319616,
    -0.00025196318894271045, 3.9347320316271636e-05,
    // db10
    0.02667005790055555, 0.18817680007769153, 0.5272011889317257, 0.6884590394536034,
    0.28117234366057847, -0.24984642432731513, -0.19594627437737813, 0.12736934033579547,
    0.09305736460356871, -0.07139414716639458, -0.02945753682187686, 0.03321267405934137,
    0.0036065535669560058, -0.01073317548333054, 0.0013953517470529002, 0.0019924052951850566,
    -0.0006858566949597118, -0.00011646685512928554, 9.35886703200696e-05, -1.3264202894521243e-05,
};

// "haar" / "db<p>", 1 <= p <= 10 -> p; 0: no such wavelet
int wavelet_order(const char *name) {
  if (!std::strcmp(name, "haar")) return 1;
  if (name[0] != 'd' || name[1] != 'b' || name[2] < '1' || name[2] > '9') return 0;
  int p = name[2] - '0';
  if (name[3] == '0' && p == 1 && !name[4]) return 10;
  return name[3] ? 0 : p;
}

int wavelet_lookup(const char *name, const double **h, long long *ntaps) {
  if (!name) return fail(PDSP_ERR_BAD_ARG, "wavelet name is null");
  const int p = wavelet_order(name);
  if (p < 1 || p > kDaubechiesMax)
    return fail(PDSP_ERR_BAD_ARG, "unknown wavelet \"%.32s\" (haar, db1 ... db10)", name);
  *h = kDaubechies + (long long)p * (p - 1);  // 2 + 4 + ... + 2 (p - 1) taps come first
  *ntaps = 2 * p;
  return PDSP_OK;
}

int check_dwt_taps(const double *h, long long ntaps) {
  if (ntaps < 2 || ntaps > kDwtMaxTaps || ntaps % 2)
    return fail(PDSP_ERR_BAD_ARG, "the scaling filter must have an even number of taps, 2 ... %lld, got %lld", kDwtMaxTaps,
                ntaps);
  if (!h) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  for (long long m = 0; m < ntaps / 2; ++m) {
    double s = 0.0;
    for (long long k = 0; k + 2 * m < ntaps; ++k) s += h[k] * h[k + 2 * m];
    if (!(std::fabs(s - (m == 0 ? 1.0 : 0.0)) <= 1e-10))
      return fail(PDSP_ERR_BAD_ARG, "the taps are not an orthonormal scaling filter: sum_k h[k] h[k + %lld] is not %d "
                  "within 1e-10", 2 * m, m == 0 ? 1 : 0);
  }
  return PDSP_OK;
}

int check_dwt_levels(int levels) {
  if (levels < 1) return fail(PDSP_ERR_BAD_ARG, "levels must be >= 1, got %d", levels);
  return PDSP_OK;
}

int check_dwt_len(long long len, int levels) {
  if (levels > 62 || len < 1 || len % (1LL << levels))
    return fail(PDSP_ERR_BAD_ARG, "len must be a positive multiple of 2^levels (levels = %d), got %lld", levels, len);
  return PDSP_OK;
}

template <typename T>
int dwt_t(const pdsp_dwt *cw, bool inverse, long long batch, const T *in, long long len, long long in_stride, T *out,
          long long out_stride, hipStream_t s) {
  if (!cw) return fail(PDSP_ERR_BAD_ARG, "dwt is null");
  pdsp_dwt *const w = const_cast<pdsp_dwt *>(cw);
  const long long f = (long long)w->hg.size() / 2;
  if (batch < 0) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 0, got %lld", batch);
  if (int rc = check_dwt_len(len, w->levels)) return rc;
  if (in_stride < len || out_stride < len)
    return fail(PDSP_ERR_BAD_ARG, "strides must be >= len = %lld, got %lld (input) and %lld (output)", len, in_stride,
                out_stride);
  long long ic = 0, oc = 0;
  if (int rc = row_extents(batch, {{in_stride, len, &ic}, {out_stride, len, &oc}})) return rc;
  if (batch == 0) return PDSP_OK;
  if (!in || !out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  DwtTile t;
  if (int rc = dwt_tile_checked(f, w->levels, len, sizeof(T), inverse, &t)) return rc;
  long long blocks = 0;
  if (__builtin_mul_overflow(batch, t.tiles, &blocks) || blocks > 0x7fffffffLL)
    return fail(PDSP_ERR_BAD_ARG, "batch too large: %lld rows of %lld tiles", batch, t.tiles);
  // resident: a workgroup loads its whole row before it stores anything, so the exact in-place call is safe.  Any other
  // overlap lets one workgroup's stores reach another's loads: byte ranges of the whole strided extents
  const bool in_place = t.resident && exact_in_place(out, out_stride, in, in_stride);
  if (!in_place && host_ranges_overlap(in, (size_t)ic * sizeof(T), out, (size_t)oc * sizeof(T)))
    return fail(PDSP_ERR_BAD_ARG, t.resident ? "output overlaps input (only out == in with equal strides may share bytes)"
                                             : "output overlaps input (rows beyond the resident path share no bytes)");
  if (int rc = require_device()) return rc;
  T *&hg = w->slot<T>();
  if (int rc = first_use_table(*w, hg, s, "tap table", [&] { return std::vector<T>(w->hg.begin(), w->hg.end()); }))
    return rc;
  DeviceGuard dg(w->device);
  PDSP_HIP_TRY(dg.err);
  return dwt_dev<T>(t, hg, (int)f, w->levels, inverse, batch, in, len, in_stride, out, out_stride, s);
}

// The host forms ride the packed features' scaffold on the cached plan of 64 points (its stream, its lock, its
// device); the transform's own object lives for the call.  Buffer: out | in.
int dwt_host(bool inverse, const double *in, long long batch, long long len, const char *name, const double *taps,
             long long ntaps, int levels, double *out) {
  pdsp_dwt *w = nullptr;
  if (int rc = pdsp_dwt_create(-1, name, taps, ntaps, levels, &w)) return rc;
  const HandleOwner<pdsp_dwt> own(w);
  if (batch < 0) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 0, got %lld", batch);
  if (int rc = check_dwt_len(len, levels)) return rc;
  long long count = 0;
  if (!host_count_ok(batch, len, &count)) return fail(PDSP_ERR_BAD_ARG, "batch %lld x length overflows", batch);
  if (batch == 0) return PDSP_OK;
  if (!in || !out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  DwtTile t;
  if (int rc = dwt_tile_checked((long long)w->hg.size() / 2, levels, len, sizeof(double), inverse, &t)) return rc;
  const size_t nx = (size_t)count;
  return packed_host_call(
      64, PDSP_WIN_RECT, 2 * nx,
      [&](pdsp_plan *, hipStream_t s, const double *, double *d) -> int {
        PDSP_HIP_TRY(hipMemcpyAsync(d + nx, in, nx * sizeof(double), hipMemcpyHostToDevice, s));
        return dwt_t<double>(w, inverse, batch, d + nx, len, len, d, len, s);
      },
      [&](const double *d) -> int {
        PDSP_HIP_TRY(hipMemcpy(out, d, nx * sizeof(double), hipMemcpyDeviceToHost));
        return PDSP_OK;
      });
}

}  // namespace pdsp_host

int pdsp_wavelet_taps(const char *name, double *out, long long *ntaps) {
  if (!ntaps) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const double *h = nullptr;
  if (int rc = wavelet_lookup(name, &h, ntaps)) return rc;
  if (out) std::memcpy(out, h, (size_t)*ntaps * sizeof(double));
  return PDSP_OK;
}

int pdsp_dwt_create(int device, const char *name_or_null, const double *taps_or_null, long long ntaps, int levels,
                    pdsp_dwt **out) {
  if (!out) return fail(PDSP_ERR_BAD_ARG, "out is null");
  *out = nullptr;
  if (int rc = check_dwt_levels(levels)) return rc;
  const double *h = taps_or_null;
  if (name_or_null) {
    if (taps_or_null) return fail(PDSP_ERR_BAD_ARG, "pass a wavelet name or taps, not both");
    if (int rc = wavelet_lookup(name_or_null, &h, &ntaps)) return rc;
  }
  if (int rc = check_dwt_taps(h, ntaps)) return rc;
  pdsp_dwt *w = new (std::nothrow) pdsp_dwt();
  if (!w) return fail(PDSP_ERR_BAD_ARG, "out of host memory");
  w->device = device < 0 ? -1 : device;
  w->levels = levels;
  w->hg.assign(h, h + ntaps);
  for (long long j = 0; j < ntaps; ++j) w->hg.push_back((j % 2 ? -1.0 : 1.0) * h[ntaps - 1 - j]);
  *out = w;
  return PDSP_OK;
}

int pdsp_dwt_destroy(pdsp_dwt *w) { return destroy_handle(w); }

long long pdsp_dwt_ntaps(const pdsp_dwt *w) { return w ? (long long)w->hg.size() / 2 : 0; }
int pdsp_dwt_levels(const pdsp_dwt *w) { return w ? w->levels : 0; }
int pdsp_dwt_taps(const pdsp_dwt *w, double *taps) {
  if (!w || !taps) return fail(PDSP_ERR_BAD_ARG, w ? "null buffer" : "dwt is null");
  std::memcpy(taps, w->hg.data(), w->hg.size() / 2 * sizeof(double));
  return PDSP_OK;
}

// The rule's own answer, whatever pdsp_set_dwt_tile says: every depth on a row the resident path holds (forward:
// len + len / 2 values within 160 KiB), the tiled path's limit beyond
int pdsp_dwt_max_levels(long long ntaps, long long len, int elem_bytes) {
  if (ntaps < 2 || ntaps > kDwtMaxTaps || ntaps % 2 || len < 1 || (elem_bytes != 4 && elem_bytes != 8)) return 0;
  int most = 0;
  while (most < 62 && len % (1LL << (most + 1)) == 0) ++most;
  if (len <= (1LL << 40) && (len + len / 2) * elem_bytes <= 163840) return most;
  const int tiled = dwt_tiled_max_levels(ntaps, (size_t)elem_bytes);
  return most < tiled ? most : tiled;
}

int pdsp_dwt_forward_f32(const pdsp_dwt *w, long long batch, const float *x, long long len, long long x_stride, float *y,
                         long long y_stride, pdsp_stream stream) {
  return dwt_t<float>(w, false, batch, x, len, x_stride, y, y_stride, (hipStream_t)stream);
}
int pdsp_dwt_forward_f64(const pdsp_dwt *w, long long batch, const double *x, long long len, long long x_stride,
                         double *y, long long y_stride, pdsp_stream stream) {
  return dwt_t<double>(w, false, batch, x, len, x_stride, y, y_stride, (hipStream_t)stream);
}
int pdsp_dwt_inverse_f32(const pdsp_dwt *w, long long batch, const float *c, long long len, long long c_stride, float *x,
                         long long x_stride, pdsp_stream stream) {
  return dwt_t<float>(w, true, batch, c, len, c_stride, x, x_stride, (hipStream_t)stream);
}
int pdsp_dwt_inverse_f64(const pdsp_dwt *w, long long batch, const double *c, long long len, long long c_stride,
                         double *x, long long x_stride, pdsp_stream stream) {
  return dwt_t<double>(w, true, batch, c, len, c_stride, x, x_stride, (hipStream_t)stream);
}

int pdsp_dwt_forward_host_f64(const double *x, long long batch, long long len, const char *name_or_null,
                              const double *taps_or_null, long long ntaps, int levels, double *y) {
  return dwt_host(false, x, batch, len, name_or_null, taps_or_null, ntaps, levels, y);
}
int pdsp_dwt_inverse_host_f64(const double *c, long long batch, long long len, const char *name_or_null,
                              const double *taps_or_null, long long ntaps, int levels, double *x) {
  return dwt_host(true, c, batch, len, name_or_null, taps_or_null, ntaps, levels, x);
}

int pdsp_set_dwt_tile(int mode) {
  const int prev = g_dwt_tile;
  if (mode >= 0 && (mode & 3) <= 2) g_dwt_tile = mode;
  return prev;
}

int pdsp_dev_dwt_tile(long long ntaps, int levels, long long len, int elem_bytes, int inverse, long long info[5]) {
  if (!info) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (ntaps < 2 || ntaps > kDwtMaxTaps || ntaps % 2)
    return fail(PDSP_ERR_BAD_ARG, "the scaling filter must have an even number of taps, 2 ... %lld, got %lld", kDwtMaxTaps,
                ntaps);
  if (int rc = check_dwt_levels(levels)) return rc;
  if (int rc = check_dwt_len(len, levels)) return rc;
  if (elem_bytes != 4 && elem_bytes != 8) return fail(PDSP_ERR_BAD_ARG, "elem_bytes must be 4 or 8, got %d", elem_bytes);
  DwtTile t;
  if (int rc = dwt_tile_checked(ntaps, levels, len, (size_t)elem_bytes, inverse != 0, &t)) return rc;
  const long long v[5] = {t.resident, t.tile, t.halo, (long long)t.lds_bytes, t.tiles};
  std::memcpy(info, v, sizeof(v));
  return PDSP_OK;
}

// ---- number-theoretic transform and exact convolution over GF(2^64 - 2^32 + 1) ---------------------------------
// A handle is its size and the table omega_N^j, j < N / 2, built on the host with the header the kernels compute with
// and uploaded on first use (TableHandle, first_use_table: one precision, so one slot, in the 8-byte list).

struct pdsp_ntt : TableHandle {
  long long n = 0;
  int log2n = 0;
  uint64_t *tw = nullptr;
};

namespace pdsp_host {

int check_ntt_size(long long n) {
  if (n < 1 || (n & (n - 1))) return fail(PDSP_ERR_SIZE_NOT_POW2, "NTT size must be power of two, got %lld", n);
  if (n < (1LL << kNttMinLog2N) || n > (1LL << kNttMaxLog2N))
    return fail(PDSP_ERR_UNSUPPORTED_SIZE, "NTT size %lld is outside %lld ... %lld", n, 1LL << kNttMinLog2N,
                1LL << kNttMaxLog2N);
  return PDSP_OK;
}

// pdsp_ntt_forward_u64 / _inverse_u64 / _conv_u64: op a pdsp::NttOp (0, 1: a_len = out_len = N, b unused; 2)
int ntt_t(const pdsp_ntt *ch, int op, long long batch, const uint64_t *a, long long a_len, long long a_stride,
          const uint64_t *b, long long b_len, long long b_stride, uint64_t *out, long long out_len,
          long long out_stride, hipStream_t s) {
  if (!ch) return fail(PDSP_ERR_BAD_ARG, "ntt is null");
  pdsp_ntt *const h = const_cast<pdsp_ntt *>(ch);
  const bool conv = op == 2;
  if (batch < 0) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 0, got %lld", batch);
  if (conv) {
    if (a_len < 1 || a_len > h->n || b_len < 1 || b_len > h->n || out_len < 1 || out_len > h->n)
      return fail(PDSP_ERR_BAD_ARG, "lengths must be 1 ... N = %lld, got %lld (a), %lld (b) and %lld (out)", h->n, a_len,
                  b_len, out_len);
    if (a_stride < a_len || out_stride < out_len || (b_stride != 0 && b_stride < b_len))
      return fail(PDSP_ERR_BAD_ARG, "strides must be >= the row lengths (b: or 0), got %lld (a), %lld (b) and %lld (out)",
                  a_stride, b_stride, out_stride);
  } else if (a_stride < h->n || out_stride < h->n) {
    return fail(PDSP_ERR_BAD_ARG, "strides must be >= N = %lld, got %lld (input) and %lld (output)", h->n, a_stride,
                out_stride);
  }
  long long ac = 0, bc = 0, oc = 0;
  if (int rc = row_extents(batch, {{a_stride, a_len, &ac}, {out_stride, out_len, &oc},
                                   {conv ? b_stride : 0, conv ? b_len : 0, &bc}}))
    return rc;
  if (batch == 0) return PDSP_OK;
  if (!a || !out || (conv && !b)) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (int rc = check_grid(ntt_blocks(h->log2n, op, batch), batch)) return rc;
  // a thread stores the positions it loaded from `a`, after its last load: out == a at equal strides is exact in place.
  // Any other shared byte lets one thread's store reach another's load.
  if ((!exact_in_place(out, out_stride, a, a_stride) && host_ranges_overlap(a, (size_t)ac * 8, out, (size_t)oc * 8)) ||
      (conv && host_ranges_overlap(b, (size_t)bc * 8, out, (size_t)oc * 8)))
    return fail(PDSP_ERR_BAD_ARG, conv ? "output overlaps an input (only out == a with equal strides may share bytes)"
                                       : "output overlaps input (only out == in with equal strides may share bytes)");
  if (int rc = require_device()) return rc;
  const int rc = first_use_table(*h, h->tw, s, "root table", [&] {  // omega_N^j, j < N / 2
    std::vector<uint64_t> w((size_t)h->n / 2);
    const uint64_t root = pdsp::gl::root(h->log2n);
    uint64_t p = 1;
    for (auto &v : w) v = p, p = pdsp::gl::mul(p, root);
    return w;
  });
  if (rc) return rc;
  DeviceGuard dg(h->device);
  PDSP_HIP_TRY(dg.err);
  return ntt_dev(h->log2n, op, batch, a, a_stride, (int)a_len, b, b_stride, (int)b_len, out, out_stride, (int)out_len,
                 h->tw, s);
}

int ntt_mul_t(long long count, const uint64_t *a, const uint64_t *b, uint64_t *out, hipStream_t s) {
  if (count < 0) return fail(PDSP_ERR_BAD_ARG, "count must be >= 0, got %lld", count);
  if (count > (LLONG_MAX / 8)) return fail(PDSP_ERR_BAD_ARG, "count %lld overflows", count);
  if (count == 0) return PDSP_OK;
  if (!a || !b || !out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const size_t bytes = (size_t)count * 8;
  if (elementwise_clash(out, a, bytes) || elementwise_clash(out, b, bytes))
    return fail(PDSP_ERR_BAD_ARG, "output overlaps input");
  if (int rc = require_device()) return rc;
  return ntt_mul_dev(count, a, b, out, s);
}

// The host forms ride the packed features' scaffold on the cached plan of 64 points (its stream, its lock, its
// device); the transform's own object lives for the call.  Buffer (8-byte values): out | a | b.
int ntt_host(int op, const uint64_t *a, long long a_len, const uint64_t *b, long long b_len, bool b_shared,
             long long batch, long long n, uint64_t *out, long long out_len) {
  pdsp_ntt *h = nullptr;
  if (int rc = pdsp_ntt_create(n, -1, &h)) return rc;
  const HandleOwner<pdsp_ntt> own(h);
  const bool conv = op == 2;
  if (batch < 0) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 0, got %lld", batch);
  if (conv && (a_len < 1 || a_len > n || b_len < 1 || b_len > n || out_len < 1 || out_len > n))
    return fail(PDSP_ERR_BAD_ARG, "lengths must be 1 ... N = %lld, got %lld (a), %lld (b) and %lld (out)", n, a_len, b_len,
                out_len);
  long long na = 0, nb = 0, no = 0;
  if (!host_count_ok(batch, a_len, &na) || !host_count_ok(b_shared ? (batch > 0) : batch, b_len, &nb) ||
      !host_count_ok(batch, out_len, &no))
    return fail(PDSP_ERR_BAD_ARG, "batch %lld x length overflows", batch);
  if (batch == 0) return PDSP_OK;
  if (!a || !out || (conv && !b)) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (!conv) nb = 0;
  return packed_host_call(
      64, PDSP_WIN_RECT, (size_t)(no + na + nb),
      [&](pdsp_plan *, hipStream_t s, const double *, double *d) -> int {
        uint64_t *const d_out = (uint64_t *)d, *const d_a = d_out + no, *const d_b = d_a + na;
        PDSP_HIP_TRY(hipMemcpyAsync(d_a, a, (size_t)na * 8, hipMemcpyHostToDevice, s));
        if (conv) PDSP_HIP_TRY(hipMemcpyAsync(d_b, b, (size_t)nb * 8, hipMemcpyHostToDevice, s));
        return ntt_t(h, op, batch, d_a, a_len, a_len, d_b, b_len, b_shared ? 0 : b_len, d_out, out_len, out_len, s);
      },
      [&](const double *d) -> int {
        PDSP_HIP_TRY(hipMemcpy(out, d, (size_t)no * 8, hipMemcpyDeviceToHost));
        return PDSP_OK;
      });
}

}  // namespace pdsp_host

int pdsp_ntt_create(long long n, int device, pdsp_ntt **out) {
  if (!out) return fail(PDSP_ERR_BAD_ARG, "out is null");
  *out = nullptr;
  if (int rc = check_ntt_size(n)) return rc;
  pdsp_ntt *h = new (std::nothrow) pdsp_ntt();
  if (!h) return fail(PDSP_ERR_BAD_ARG, "out of host memory");
  h->n = n;
  h->log2n = ilog2ll(n);
  h->device = device < 0 ? -1 : device;
  *out = h;
  return PDSP_OK;
}

int pdsp_ntt_destroy(pdsp_ntt *h) { return destroy_handle(h); }

long long pdsp_ntt_size(const pdsp_ntt *h) { return h ? h->n : 0; }

int pdsp_ntt_forward_u64(const pdsp_ntt *h, long long batch, const uint64_t *in, long long in_stride, uint64_t *out,
                         long long out_stride, pdsp_stream stream) {
  const long long n = h ? h->n : 0;
  return ntt_t(h, 0, batch, in, n, in_stride, nullptr, 0, 0, out, n, out_stride, (hipStream_t)stream);
}
int pdsp_ntt_inverse_u64(const pdsp_ntt *h, long long batch, const uint64_t *in, long long in_stride, uint64_t *out,
                         long long out_stride, pdsp_stream stream) {
  const long long n = h ? h->n : 0;
  return ntt_t(h, 1, batch, in, n, in_stride, nullptr, 0, 0, out, n, out_stride, (hipStream_t)stream);
}
int pdsp_ntt_conv_u64(const pdsp_ntt *h, long long batch, const uint64_t *a, long long a_len, long long a_stride,
                      const uint64_t *b, long long b_len, long long b_stride, uint64_t *out, long long out_len,
                      long long out_stride, pdsp_stream stream) {
  return ntt_t(h, 2, batch, a, a_len, a_stride, b, b_len, b_stride, out, out_len, out_stride, (hipStream_t)stream);
}
int pdsp_ntt_mul_u64(long long count, const uint64_t *a, const uint64_t *b, uint64_t *out, pdsp_stream stream) {
  return ntt_mul_t(count, a, b, out, (hipStream_t)stream);
}

int pdsp_ntt_host_u64(const uint64_t *x, long long batch, long long n, int inverse, uint64_t *out) {
  return ntt_host(inverse ? 1 : 0, x, n, nullptr, 0, false, batch, n, out, n);
}
int pdsp_ntt_conv_host_u64(const uint64_t *a, long long a_len, const uint64_t *b, long long b_len, int b_shared,
                           long long batch, long long n, uint64_t *out, long long out_len) {
  return ntt_host(2, a, a_len, b, b_len, b_shared != 0, batch, n, out, out_len);
}

uint64_t pdsp_ntt_modulus(void) { return pdsp::gl::kP; }
uint64_t pdsp_ntt_root(long long n) {
  if (n < 1 || (n & (n - 1)) || n > (1LL << pdsp::gl::kMaxLog2Root)) return 0;
  return pdsp::gl::root(ilog2ll(n));
}
uint64_t pdsp_ntt_mulmod(uint64_t a, uint64_t b) { return pdsp::gl::mul(pdsp::gl::canon(a), pdsp::gl::canon(b)); }
uint64_t pdsp_ntt_powmod(uint64_t a, uint64_t e) { return pdsp::gl::pow(pdsp::gl::canon(a), e); }
uint64_t pdsp_ntt_invmod(uint64_t a) { return pdsp::gl::inv(pdsp::gl::canon(a)); }

// ---- sliding DFT: chosen bins at every hop ----------------------------------------------------------------------
// A handle is its phase tables: per bin and component the N + 1 entries exp(-2 pi i (t1 +- t2)) of
// include/pdsp_hip.h, evaluated in long double on the host from exactly reduced phases and rounded once per precision.
// They go up at create time through the plans' uploader into the handle's own lists (TableHandle).

struct pdsp_sdft : TableHandle {
  long long n = 0, hop = 0;
  int nbins = 0, ncomp = 0, window = 0;
  std::vector<double> bins;
  double weights[5] = {0, 0, 0, 0, 0};
  float2 *tab32 = nullptr;
  double2 *tab64 = nullptr;
  template <typename T>
  auto slot() const {
    if constexpr (sizeof(T) == 4) return (const float2 *)tab32;
    else return (const double2 *)tab64;
  }
};

namespace pdsp_host {

constexpr long long kSdftMaxLen = 16384, kSdftMaxBins = 256, kSdftMaxTable = 1LL << 21;

// The window as a cosine sum in 2 pi n / (N - 1): a_0, then (-1)^c a_c / 2 for the components (b + c N / (N - 1)) and
// (b - c N / (N - 1)), c = 1, 2.  Returns the number of components, 0 for an unknown type.
int sdft_weights(int window_type, double w[5]) {
  for (int i = 0; i < 5; ++i) w[i] = 0.0;
  switch (window_type) {
    case PDSP_WIN_RECT: w[0] = 1.0; return 1;
    case PDSP_WIN_HANN: w[0] = 0.5, w[1] = w[2] = -0.25; return 3;
    case PDSP_WIN_HAMMING: w[0] = 0.54, w[1] = w[2] = -0.23; return 3;
    case PDSP_WIN_BLACKMAN: w[0] = 0.42, w[1] = w[2] = -0.25, w[3] = w[4] = 0.04; return 5;
  }
  return 0;
}

int check_sdft_args(long long n, long long nbins, const double *bins, long long hop, int window_type) {
  if (n < 2 || n > kSdftMaxLen)
    return fail(PDSP_ERR_UNSUPPORTED_SIZE, "sliding DFT window length must be 2 ... %lld, got %lld", kSdftMaxLen, n);
  if (nbins < 1 || nbins > kSdftMaxBins)
    return fail(PDSP_ERR_UNSUPPORTED_SIZE, "sliding DFT bins must be 1 ... %lld, got %lld", kSdftMaxBins, nbins);
  if (hop < 1) return fail(PDSP_ERR_BAD_ARG, "hop must be >= 1, got %lld", hop);
  double w[5];
  const int ncomp = sdft_weights(window_type, w);
  if (!ncomp) return fail(PDSP_ERR_BAD_ARG, "Unsupported window type: %d", window_type);
  if (!bins) return fail(PDSP_ERR_BAD_ARG, "bins is null");
  // (a double of 2^53 or more is a whole number of cycles)
  for (long long j = 0; j < nbins; ++j)
    if (!(std::fabs(bins[j]) < 0x1p53))
      return fail(PDSP_ERR_BAD_ARG, "sliding DFT bins must be finite and below 2^53 in magnitude, got %g at index %lld",
                  bins[j], j);
  if (nbins * ncomp * (n + 1) > kSdftMaxTable)
    return fail(PDSP_ERR_UNSUPPORTED_SIZE,
                "sliding DFT tables of %lld bins x %d components x %lld entries exceed 2^21 entries", nbins, ncomp,
                n + 1);
  return PDSP_OK;
}

// exp(-2 pi i (t1 + sign t2)) at position i: t1 = ((b i) mod N) / N by czt_turns' rule (error-free product, fmod, the
// error term added after the reduction) and brought into [0, N) -- fmod keeps the sign of a negative bin, and b and
// b + N must meet in one table --, t2 = ((c i) mod (N - 1)) / (N - 1) in integers
ldcx sdft_phase(long long n, double bin, int c, long long i) {
  long double r = czt_turns(i, bin, (double)n);
  if (r < 0.0L) r += (long double)n;
  long double t = r / (long double)n;
  if (c != 0) {
    const long long ac = c < 0 ? -c : c;
    const long double t2 = (long double)((ac * i) % (n - 1)) / (long double)(n - 1);
    t += c < 0 ? -t2 : t2;
  }
  const long double a = -2.0L * kPiL * t;
  return ldcx{cosl(a), sinl(a)};
}

// component k of the table order: 0, +1, -1, +2, -2
constexpr int sdft_component(int k) { return k == 0 ? 0 : (k & 1 ? (k + 1) / 2 : -(k / 2)); }

long long sdft_frames(long long n, long long hop, long long samples) {
  return samples < n ? 0 : 1 + (samples - n) / hop;
}

template <typename T>
int sdft_t(const pdsp_sdft *c, long long batch, const T *in, long long in_stride, long long samples, T *re_out,
           T *im_out, long long out_stride, hipStream_t s) {
  if (!c) return fail(PDSP_ERR_BAD_ARG, "sdft is null");
  if (batch < 1) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 1, got %lld", batch);
  if (samples < c->n)
    return fail(PDSP_ERR_INPUT_LENGTH, "sliding DFT rows of %lld samples are shorter than the window of %lld", samples,
                c->n);
  const long long frames = sdft_frames(c->n, c->hop, samples);
  if (in_stride < samples || out_stride < frames)
    return fail(PDSP_ERR_BAD_ARG,
                "strides must be >= %lld samples in and >= %lld frames out, got in_stride %lld, out_stride %lld", samples,
                frames, in_stride, out_stride);
  long long ic = 0, oc = 0;  // a plane of the output holds one series of frames per bin and row
  if (int rc = row_extents(batch, {{in_stride, samples, &ic}, {out_stride, frames, &oc, c->nbins}})) return rc;
  if (!in || !re_out || !im_out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const long long blocks = sdft_blocks(c->n, sizeof(T), samples, c->nbins, batch);
  if (blocks < 0 || blocks > 0x7fffffffLL) return fail(PDSP_ERR_BAD_ARG, "batch too large: %lld", batch);
  // no in-place form: a workgroup reads samples that other workgroups' frames are stored over
  const size_t ib = (size_t)ic * sizeof(T), ob = (size_t)oc * sizeof(T);
  if (host_ranges_overlap(re_out, ob, in, ib) || host_ranges_overlap(im_out, ob, in, ib))
    return fail(PDSP_ERR_BAD_ARG, "output overlaps input (the sliding DFT has no in-place form)");
  if (host_ranges_overlap(re_out, ob, im_out, ob))
    return fail(PDSP_ERR_BAD_ARG, "the output planes overlap each other");
  DeviceGuard dg(c->device);
  PDSP_HIP_TRY(dg.err);
  return sdft_dev<T>(c->n, c->hop, c->nbins, c->ncomp, c->weights, batch, in, in_stride, samples, re_out, im_out,
                     out_stride, c->slot<T>(), s);
}

}  // namespace pdsp_host

int pdsp_sdft_create(long long window_len, long long nbins, const double *bins, long long hop, int window_type,
                     int device, pdsp_sdft **out) {
  if (!out) return fail(PDSP_ERR_BAD_ARG, "out is null");
  if (int rc = check_sdft_args(window_len, nbins, bins, hop, window_type)) return rc;
  if (int rc = require_device()) return rc;
  if (int rc = resolve_device(&device)) return rc;
  DeviceGuard g(device);
  PDSP_HIP_TRY(g.err);
  pdsp_sdft *c = new (std::nothrow) pdsp_sdft();
  if (!c) return fail(PDSP_ERR_BAD_ARG, "out of host memory");
  c->device = device, c->n = window_len, c->hop = hop, c->nbins = (int)nbins, c->window = window_type;
  c->ncomp = sdft_weights(window_type, c->weights);
  c->bins.assign(bins, bins + nbins);
  const long long per = window_len + 1;
  std::vector<double2> tab((size_t)(nbins * c->ncomp * per));
  std::vector<float2> tabf(tab.size());  // each precision rounded once, from the long double
  for (long long j = 0; j < nbins; ++j)
    for (int k = 0; k < c->ncomp; ++k) {
      const size_t at = (size_t)((j * c->ncomp + k) * per);
      for (long long i = 0; i < per; ++i) {
        const ldcx v = sdft_phase(window_len, bins[j], sdft_component(k), i);
        tab[at + (size_t)i] = double2{(double)v.x, (double)v.y};
        tabf[at + (size_t)i] = float2{(float)v.x, (float)v.y};
      }
    }
  hipError_t e = upload_table(c->t32, tabf, &c->tab32);
  if (e == hipSuccess) e = upload_table(c->t64, tab, &c->tab64);
  if (e != hipSuccess) {
    pdsp_sdft_destroy(c);
    return fail(PDSP_ERR_DEVICE, "HIP error %d (%s) at hipMalloc / hipMemcpy of the sliding DFT tables", (int)e,
                hipGetErrorString(e));
  }
  *out = c;
  return PDSP_OK;
}

int pdsp_sdft_destroy(pdsp_sdft *c) { return destroy_handle(c); }

long long pdsp_sdft_length(const pdsp_sdft *c) { return c ? c->n : 0; }
long long pdsp_sdft_bins(const pdsp_sdft *c) { return c ? c->nbins : 0; }
long long pdsp_sdft_hop(const pdsp_sdft *c) { return c ? c->hop : 0; }
long long pdsp_sdft_components(const pdsp_sdft *c) { return c ? c->ncomp : 0; }
double pdsp_sdft_bin(const pdsp_sdft *c, long long index) {
  return c && index >= 0 && index < c->nbins ? c->bins[(size_t)index] : 0.0;
}
long long pdsp_sdft_frames(const pdsp_sdft *c, long long samples) {
  return c ? sdft_frames(c->n, c->hop, samples) : 0;
}

int pdsp_sdft_window_weights(int window_type, double weights[5]) {
  if (!weights) return fail(PDSP_ERR_BAD_ARG, "weights is null"), 0;
  const int ncomp = sdft_weights(window_type, weights);
  if (!ncomp) fail(PDSP_ERR_BAD_ARG, "Unsupported window type: %d", window_type);
  return ncomp;
}

int pdsp_sdft_phase_table(long long window_len, double bin, int component, double *re_out, double *im_out) {
  const double b[1] = {bin};
  if (int rc = check_sdft_args(window_len, 1, b, 1, PDSP_WIN_RECT)) return rc;
  if (component < -2 || component > 2) return fail(PDSP_ERR_BAD_ARG, "component must be -2 ... 2, got %d", component);
  if (!re_out || !im_out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  for (long long i = 0; i <= window_len; ++i) {
    const ldcx v = sdft_phase(window_len, bin, component, i);
    re_out[i] = (double)v.x, im_out[i] = (double)v.y;
  }
  return PDSP_OK;
}

int pdsp_sdft_f32(const pdsp_sdft *c, long long batch, const float *in, long long in_stride, long long samples,
                  float *re_out, float *im_out, long long out_stride, pdsp_stream stream) {
  return sdft_t<float>(c, batch, in, in_stride, samples, re_out, im_out, out_stride, (hipStream_t)stream);
}
int pdsp_sdft_f64(const pdsp_sdft *c, long long batch, const double *in, long long in_stride, long long samples,
                  double *re_out, double *im_out, long long out_stride, pdsp_stream stream) {
  return sdft_t<double>(c, batch, in, in_stride, samples, re_out, im_out, out_stride, (hipStream_t)stream);
}

// The host form rides the packed features' scaffold on the cached plan of 64 points (its stream, its lock, its
// device), as the NTT's does; the handle lives for the call.  Buffer: out re | out im | in.
int pdsp_sdft_host_f64(const double *in, long long batch, long long samples, long long window_len, long long nbins,
                       const double *bins, long long hop, int window_type, double *re_out, double *im_out) {
  if (int rc = check_sdft_args(window_len, nbins, bins, hop, window_type)) return rc;
  if (batch < 1) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 1, got %lld", batch);
  if (samples < window_len)
    return fail(PDSP_ERR_INPUT_LENGTH, "sliding DFT rows of %lld samples are shorter than the window of %lld", samples,
                window_len);
  const long long frames = sdft_frames(window_len, hop, samples);
  long long cin = 0, series = 0, cout = 0;
  if (!host_count_ok(batch, samples, &cin) || !host_count_ok(batch, nbins, &series) ||
      !host_count_ok(series, frames, &cout))
    return fail(PDSP_ERR_BAD_ARG, "batch %lld x (%lld, %lld) overflows", batch, samples, frames);
  if (!in || !re_out || !im_out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  const size_t nx = (size_t)cin, ny = (size_t)cout;
  HandleOwner<pdsp_sdft> own;
  return packed_host_call(
      64, PDSP_WIN_RECT, 2 * ny + nx,
      [&](pdsp_plan *plan, hipStream_t s, const double *, double *d) -> int {
        pdsp_sdft *c = nullptr;
        if (int rc = pdsp_sdft_create(window_len, nbins, bins, hop, window_type, plan->device, &c)) return rc;
        own.reset(c);
        double *const x = d + 2 * ny;
        PDSP_HIP_TRY(hipMemcpyAsync(x, in, nx * sizeof(double), hipMemcpyHostToDevice, s));
        return sdft_t<double>(c, batch, x, samples, samples, d, d + ny, frames, s);
      },
      [&](const double *d) -> int {
        PDSP_HIP_TRY(hipMemcpy(re_out, d, ny * sizeof(double), hipMemcpyDeviceToHost));
        PDSP_HIP_TRY(hipMemcpy(im_out, d + ny, ny * sizeof(double), hipMemcpyDeviceToHost));
        return PDSP_OK;
      });
}

/* ---- 2-D transform of images: fft2 / ifft2 (include/pdsp_hip_fft2d.h) --------- */

// A 2-D transform has no table of its own: the object borrows the cached plans of W and H points on its device and
// keeps them pinned while it lives (a pinned entry is never evicted and survives pdsp_plan_cache_clear), so every
// table it needs is on the device when create returns.  Built on TableHandle for the device and destroy_handle; its
// own lists of allocations stay empty.
struct pdsp_fft2d : TableHandle {
  long long h = 0, w = 0;
  CachedPlan plan_w, plan_h;
};

namespace pdsp_host {

int fft2d_shape(long long height, long long width, size_t elem, Fft2dPath *path) {
  if (fft2d_path(height, width, elem, path)) return PDSP_OK;
  return fail(PDSP_ERR_UNSUPPORTED_SIZE,
              "2-D FFT images must be H x W with H and W powers of two, 16 <= H <= 512, 16 <= W <= %d in f32 and %d in "
              "f64, got %lld x %lld (%d-byte scalars)",
              1 << pdsp::kMaxLog2N_f32, 1 << pdsp::kMaxLog2N_f64, height, width, (int)elem);
}

int check_fft2d_norm(int norm) {
  if (norm < PDSP_NORM_BACKWARD || norm > PDSP_NORM_FORWARD)
    return fail(PDSP_ERR_BAD_ARG, "2-D FFT norm must be 0 (backward), 1 (ortho) or 2 (forward), got %d", norm);
  return PDSP_OK;
}

// numpy's norm as the one scale of the last store, computed in f64 and rounded once (H W is a power of two: 1 / (H W)
// is exact, and 1 / sqrt(H W) is where log2(H W) is even)
double fft2d_scale(long long hw, int inverse, int norm) {
  if (norm == PDSP_NORM_ORTHO) return 1.0 / std::sqrt((double)hw);
  return (norm == PDSP_NORM_FORWARD) != (inverse != 0) ? 1.0 / (double)hw : 1.0;
}

// The argument checks of one call, ahead of the device; then the launch.  Exact in place is the one overlap allowed
// (the header's aliasing rule); the inverse is the forward transform of the swapped planes, so the rule is the same.
template <typename T>
int fft2d_t(const pdsp_fft2d *f, long long batch, const T *re_in, const T *im_in, T *re_out, T *im_out, int inverse,
            int norm, hipStream_t s) {
  if (!f) return fail(PDSP_ERR_BAD_ARG, "fft2d is null");
  if (batch < 1) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 1, got %lld", batch);
  if (int rc = check_fft2d_norm(norm)) return rc;
  if (!re_in || !re_out || !im_out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (inverse && !im_in) return fail(PDSP_ERR_BAD_ARG, "the inverse needs both planes (im_in is null)");
  Fft2dPath path;
  if (int rc = fft2d_shape(f->h, f->w, sizeof(T), &path)) return rc;
  long long count = 0;
  if (!mad_ok(batch, f->h * f->w, 0, &count) || count > (LLONG_MAX / 8))
    return fail(PDSP_ERR_BAD_ARG, "batch %lld x H x W overflows", batch);
  if ((((uintptr_t)re_in | (uintptr_t)im_in | (uintptr_t)re_out | (uintptr_t)im_out) & 15) != 0)
    return fail(PDSP_ERR_BAD_ARG, "the planes must begin on 16-byte boundaries");
  const size_t bytes = (size_t)count * sizeof(T);
  const bool in_place = re_out == re_in && (!im_in || im_out == im_in);
  if (!in_place && (host_ranges_overlap(re_out, bytes, re_in, bytes) || host_ranges_overlap(re_out, bytes, im_in, bytes) ||
                    host_ranges_overlap(im_out, bytes, re_in, bytes) || host_ranges_overlap(im_out, bytes, im_in, bytes)))
    return fail(PDSP_ERR_BAD_ARG, "output overlaps input (only re_out == re_in with im_out == im_in, or with a null "
                                  "im_in, may share bytes)");
  if (host_ranges_overlap(re_out, bytes, im_out, bytes))
    return fail(PDSP_ERR_BAD_ARG, "the output planes overlap each other");
  DeviceGuard dg(f->device);
  PDSP_HIP_TRY(dg.err);
  const T scale = (T)fft2d_scale(f->h * f->w, inverse, norm);
  if (inverse)
    return fft2d_dev<T>(path, f->plan_w.plan, f->plan_h.plan, batch, im_in, re_in, im_out, re_out, scale, s);
  return fft2d_dev<T>(path, f->plan_w.plan, f->plan_h.plan, batch, re_in, im_in, re_out, im_out, scale, s);
}

}  // namespace pdsp_host

int pdsp_fft2d_create(long long height, long long width, int device, pdsp_fft2d **out) {
  if (!out) return fail(PDSP_ERR_BAD_ARG, "out is null");
  Fft2dPath path;
  if (int rc = fft2d_shape(height, width, 4, &path)) return rc;  // the f32 domain holds the f64 one
  if (int rc = require_device()) return rc;
  if (int rc = resolve_device(&device)) return rc;
  DeviceGuard g(device);  // cached_plan asks for the current device's plans
  PDSP_HIP_TRY(g.err);
  HandleOwner<pdsp_fft2d> f(new (std::nothrow) pdsp_fft2d());
  if (!f) return fail(PDSP_ERR_BAD_ARG, "out of host memory");
  f->device = device, f->h = height, f->w = width;
  if (int rc = cached_plan(width, &f->plan_w)) return rc;
  if (int rc = cached_plan(height, &f->plan_h)) return rc;
  *out = f.release();
  return PDSP_OK;
}

int pdsp_fft2d_destroy(pdsp_fft2d *f) { return destroy_handle(f); }
long long pdsp_fft2d_height(const pdsp_fft2d *f) { return f ? f->h : 0; }
long long pdsp_fft2d_width(const pdsp_fft2d *f) { return f ? f->w : 0; }

int pdsp_fft2d_c2c_f32(const pdsp_fft2d *f, long long batch, const float *re_in, const float *im_in, float *re_out,
                       float *im_out, int inverse, int norm, pdsp_stream stream) {
  return fft2d_t<float>(f, batch, re_in, im_in, re_out, im_out, inverse, norm, (hipStream_t)stream);
}
int pdsp_fft2d_c2c_f64(const pdsp_fft2d *f, long long batch, const double *re_in, const double *im_in, double *re_out,
                       double *im_out, int inverse, int norm, pdsp_stream stream) {
  return fft2d_t<double>(f, batch, re_in, im_in, re_out, im_out, inverse, norm, (hipStream_t)stream);
}

int pdsp_fft2d_query(long long height, long long width, int scalar_bytes, int info[PDSP_FFT2D_INFO]) {
  if (!info) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (scalar_bytes != 4 && scalar_bytes != 8)
    return fail(PDSP_ERR_BAD_ARG, "scalar_bytes must be 4 or 8, got %d", scalar_bytes);
  Fft2dPath path;
  if (int rc = fft2d_shape(height, width, (size_t)scalar_bytes, &path)) return rc;
  info[0] = path.resident ? PDSP_FFT2D_RESIDENT : PDSP_FFT2D_TWO_PASS;
  info[1] = path.images, info[2] = path.tile, info[3] = path.launches;
  return PDSP_OK;
}

// The host form rides the packed features' scaffold on the cached plan of W points (its stream, its lock, its device).
// Its checks come in the stream entry points' order (batch, norm, buffers, then the shape).  The object lives for the
// call; it is made before the scaffold takes the W-plan's lock and destroyed after that lock is released, so no lock
// of the plan cache is ever taken under a plan's.  Buffer: re | im, transformed in place (a real image's zero plane is
// written here).
int pdsp_fft2d_host_f64(const double *re_in, const double *im_in, long long batch, long long height, long long width,
                        int inverse, int norm, double *re_out, double *im_out) {
  if (batch < 1) return fail(PDSP_ERR_BAD_ARG, "batch must be >= 1, got %lld", batch);
  if (int rc = check_fft2d_norm(norm)) return rc;
  if (!re_in || !re_out || !im_out) return fail(PDSP_ERR_BAD_ARG, "null buffer");
  if (inverse && !im_in) return fail(PDSP_ERR_BAD_ARG, "the inverse needs both planes (im_in is null)");
  Fft2dPath path;
  if (int rc = fft2d_shape(height, width, sizeof(double), &path)) return rc;
  long long count = 0;
  if (batch > 0x7fffffffLL || !host_count_ok(batch, height * width, &count))
    return fail(PDSP_ERR_BAD_ARG, "batch %lld x (%lld, %lld) overflows", batch, height, width);
  const size_t n = (size_t)count;
  pdsp_fft2d *made = nullptr;
  if (int rc = pdsp_fft2d_create(height, width, -1, &made)) return rc;  // the current device: the scaffold's too
  const HandleOwner<pdsp_fft2d> own(made);
  const pdsp_fft2d *const f = made;
  return packed_host_call(
      width, PDSP_WIN_RECT, 2 * n,
      [&](pdsp_plan *, hipStream_t s, const double *, double *d) -> int {
        PDSP_HIP_TRY(hipMemcpyAsync(d, re_in, n * sizeof(double), hipMemcpyHostToDevice, s));
        if (im_in) PDSP_HIP_TRY(hipMemcpyAsync(d + n, im_in, n * sizeof(double), hipMemcpyHostToDevice, s));
        return fft2d_t<double>(f, batch, d, im_in ? d + n : nullptr, d, d + n, inverse, norm, s);
      },
      [&](const double *d) -> int {
        PDSP_HIP_TRY(hipMemcpy(re_out, d, n * sizeof(double), hipMemcpyDeviceToHost));
        PDSP_HIP_TRY(hipMemcpy(im_out, d + n, n * sizeof(double), hipMemcpyDeviceToHost));
        return PDSP_OK;
      });
}

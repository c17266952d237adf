// pdsp_host.h -- what the host units of libpdsp_hip.so (pdsp_capi*.hip) share and no kernel unit needs: the pin of a
// cached plan, the table uploader and the handles that own tables, the row-extent and overlap checks of the argument
// validators, the scaffold of the stream-ordered host forms, and the DECLARATIONS of the helpers that are defined once,
// in pdsp_capi.hip.  Included by the pdsp_capi*.hip units only: no pdsp_kernels_*.hip, kernel header or
// pdsp_dispatch.inc includes it, so a change here recompiles no kernel (pdsp_internal.h is the contract between the
// two sides).  Everything here is in namespace pdsp_host -- shared across units; what one unit alone uses stays in that
// unit, in an anonymous namespace.
#pragma once
#include <cmath>
#include <initializer_list>
#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "pdsp_internal.h"

namespace pdsp_host {

// the calling thread's error text behind fail() (defined in pdsp_capi.hip): run_chunked carries a worker's text to the caller
extern thread_local std::string g_err;

// ---- devices (defined in pdsp_capi.hip) ---------------------------------------------------------------------
int require_device();
int resolve_device(int *device);
int refuse_upload_in_capture(hipStream_t s, const char *what);

// ---- plans: stream, staging and the plan cache (defined in pdsp_capi.hip) ------------------------------------
int ensure_plan_stream(pdsp_plan *plan);
int ensure_stage(pdsp_plan *plan, size_t bytes);
void trim_stage(pdsp_plan *plan);

// The cache of pdsp_capi.hip (cached_plan), visible here for CachedPlan's destructor.
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
PlanCache &plan_cache();

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

int cached_plan(long long n, CachedPlan *out);

// ---- plan and handle tables -----------------------------------------------------------------------------------
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

// ---- operands of a call ---------------------------------------------------------------------------------------
// One strided operand of a row call: rows of `len` elements, `stride` elements apart, `per_batch` of them for each row
// of the call (the sliding DFT's series: one per bin).  *count receives its extent in elements, from the first element
// of the first row to the last of the last: (rows - 1) * stride + len.
struct RowExtent {
  long long stride, len;
  long long *count;
  long long per_batch = 1;
};
int row_extents(long long batch, std::initializer_list<RowExtent> operands);  // defined in pdsp_capi.hip
// The host forms' twin: batch contiguous rows of len values, at most 2^40 of them (the caller words the refusal).
inline bool host_count_ok(long long batch, long long len, long long *count) {
  return mad_ok(batch, len, 0, count) && *count <= (1LL << 40);
}

// The element-wise kernels read index i of every input before they write index i and touch no other index, so an
// output may share bytes with an input of the same extent only where the two begin at the same address.
inline bool elementwise_clash(const void *out, const void *in, size_t bytes) {
  return out != in && host_ranges_overlap(out, bytes, in, bytes);
}

// ---- the packed-real features and the scaffold of the stream-ordered host forms -------------------------------
int packed_size_error(const char *what, long long n);  // defined in pdsp_capi.hip
template <typename T>
int check_packed_plan(const pdsp_plan *plan, const char *what, bool need_tw4n) {
  if (!plan) return fail(PDSP_ERR_BAD_ARG, "plan is null");
  const Tables<T> &t = tables<T>(plan);
  if (plan->log2n < 6 || plan->log2n > pdsp::kMaxLog2N_f32 || !t.tw_half || !t.twr || (need_tw4n && !t.tw4n))
    return packed_size_error(what, plan->n);
  return PDSP_OK;
}

int check_packed_size(long long n, const char *what);  // defined in pdsp_capi.hip

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

// ---- phases in long double (the chirp tables and the sliding DFT's) -------------------------------------------
constexpr long double kPiL = 3.141592653589793238462643383279502884L;

// The tables are evaluated in long double from exactly reduced phases.  (n t) mod `mod` in turns, exactly: n an integer
// below 2^27 (or its square), t the caller's double.  p + e is the product without error; fmod of p is exact; the error
// term is added after the reduction, so the sum carries the product's low bits however large n t is.
inline long double czt_turns(long long n, double t, double mod) {
  const double p = (double)n * t, e = std::fma((double)n, t, -p);
  return (long double)std::fmod(p, mod) + (long double)e;
}

struct ldcx {
  long double x, y;
};

}  // namespace pdsp_host

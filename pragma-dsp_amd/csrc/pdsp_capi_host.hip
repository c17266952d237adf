// pdsp_capi_host.hip -- the f64 drop-in: the synchronous host-f64 entry points of transforms, spectra and the
// element-wise helpers that the JS drop-in binds, with the chunked host calls behind them (run_chunked), their
// pdsp_dev_host_*_chunks queries and pdsp_set_host_precision.  Calls run_complex, spectrum_impl, apply_window_dev and
// polar_dev (pdsp_kernels_f32_fft / _f32_spectrum / _f64); the plan, its stream and staging come from pdsp_capi.hip.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <atomic>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "pdsp_host.h"

using namespace pdsp_host;

namespace {

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

extern "C" {

int pdsp_set_host_precision(int bits) {
  const int prev = host_precision();
  if (bits == 32 || bits == 64) g_host_precision = bits;
  return prev;
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

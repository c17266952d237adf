// pdsp_peaks.h -- findPeak on the device: the record, the merge rule, and the kernels that search stored rows.
#pragma once

#include "pdsp_fft_core.h"

namespace pdsp {

// SpectrumPeak per frame (src/public/spectrum.ts:15-20) in f32; layout == pdsp_peak32.
struct PeakRec {
  int index;
  float frequency;
  float amplitude;
  float phase;
};

// THE merge rule of findPeak (spectrum.ts:74-105) over bins >= 1, on (value, index) pairs: does (ov, oi) replace
// (v, i)?  A larger value wins; an equal value wins only with a smaller index ("strict >, first wins", made
// order-independent); only values > 0 ever enter, and index 0 means "no bin > 0 yet".
// Every holder keeps  i == 0 <=> v == 0:  it starts at (0, 0), amplitudes are >= 0 and never NaN when they enter
// (a NaN fails every '>'), and a pair is replaced only through '>' over a value >= 0 or through this rule, i.e. by
// a value > 0 with the index >= 1 of its bin.  So the spelling  oi != 0 && (i == 0 || oi < i)  of the tie was the
// same predicate:  ov == v > 0: both indices are non-zero and it reduces to  oi < i;  ov == v == 0: both are zero
// and  oi != 0  fails as  ov > 0  does.  (A value 0 at an index > 0, which PeakBest::consider_descending may hand
// over, fails both '>' here.)  The `if` lives here and the caller passes what winning does: as a predicate returning
// bool the rule compiles branch-free and loads the holder's index eagerly, one more VGPR in the row kernels.
template <typename T, class F>
__device__ __forceinline__ void peak_if_wins(const T ov, const int oi, const T v, const int i, F &&take) {
  if (ov > v || (ov == v && ov > T(0) && oi < i)) take();
}

// Running arg-max under that rule.
template <typename T>
struct PeakBest {
  T v;
  int i;
  cx<T> x;  // the complex bin, so the phase is one atan2 at the very end
  __device__ __forceinline__ void take_if(const bool wins, const T ov, const int oi, const cx<T> ox) {
    if (wins) v = ov, i = oi, x = ox;
  }
  __device__ __forceinline__ void consider(const T ov, const int oi, const cx<T> ox) {
    peak_if_wins(ov, oi, v, i, [&] { v = ov, i = oi, x = ox; });
  }
  // A thread that visits its OWN bins in a known index order does not need the order-independent rule: in ASCENDING
  // order the strict '>' alone is "first wins" (an equal value at a larger index never replaces), in DESCENDING order
  // '>=' is (an equal value at a smaller index does replace).  One compare + four selects per bin where the rule
  // above costs four compares and their mask logic -- 32 bins per thread in the N = 16384 kernel, on a peaks-only
  // path that is bound by instruction issue, not by HBM.  A descending run may pick up a bin of value 0; the
  // order-independent merge that follows drops it (only values > 0 enter).  NaNs never enter, as before.
  __device__ __forceinline__ void consider_ascending(const T ov, const int oi, const cx<T> ox) {
    take_if(ov > v, ov, oi, ox);
  }
  __device__ __forceinline__ void consider_descending(const T ov, const int oi, const cx<T> ox) {
    take_if(ov >= v, ov, oi, ox);
  }
};

// The record of a fused spectrum kernel: `best` over bins >= 1, DC kept apart.
template <typename T>
__device__ __forceinline__ void store_peak_fused(PeakRec *__restrict__ peaks, const long long row, const PeakBest<T> &best,
                                                 const T dc_amp, const cx<T> dc_x, const T freq_scale) {
  // nothing > 0 beyond DC: findPeak falls back to the global max, which is bin 0
  const bool none = best.i == 0;
  const cx<T> px = none ? dc_x : best.x;
  PeakRec r;
  r.index = best.i;
  r.frequency = (float)(T(best.i) * freq_scale);
  r.amplitude = (float)(none ? dc_amp : best.v);
  r.phase = (float)atan2(px.y, px.x);
  peaks[row] = r;
}

// The record of a row kernel: amplitude and phase read back from the stored rows (a = the row's amplitudes).
template <typename T>
__device__ __forceinline__ void store_peak_from_row(PeakRec *__restrict__ peaks, const long long row, const int idx,
                                                    const T *a, const T *__restrict__ ph, const int bins, const T freq_scale) {
  PeakRec r;
  r.index = idx;
  r.frequency = (float)(T(idx) * freq_scale);
  r.amplitude = (float)a[idx];
  r.phase = ph ? (float)ph[(size_t)row * (size_t)bins + idx] : 0.0f;
  peaks[row] = r;
}

// One thread's bins 1 + first, 1 + first + STRIDE, ... of a stored row: strict '>', the earliest index wins.
template <typename T, int STRIDE>
__device__ __forceinline__ void peak_scan(const T *a, const int bins, const int first, T &best_v, int &best_i) {
  T bv = T(0);
  int bi = 0;
  for (int i = 1 + first; i < bins; i += STRIDE) {
    const T v = a[i];
    if (v > bv) {
      bv = v;
      bi = i;
    }
  }
  best_v = bv, best_i = bi;
}

// findPeak of one stored row by a 256-thread workgroup: strided scan, then a reduction through LDS.  Thread 0 hands
// done(idx) the first bin >= 1 holding the largest value > 0, or 0 (the reference's global-max fallback: bin 0).
template <typename T, class F>
__device__ __forceinline__ void peak_of_row(const T *a, const int bins, F &&done) {
  __shared__ T sv[256];
  __shared__ int si[256];
  T bv;
  int bi;
  peak_scan<T, 256>(a, bins, (int)threadIdx.x, bv, bi);
  sv[threadIdx.x] = bv;
  si[threadIdx.x] = bi;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const T ov = sv[threadIdx.x + s], mv = sv[threadIdx.x];
      const int oi = si[threadIdx.x + s], mi = si[threadIdx.x];
      peak_if_wins(ov, oi, mv, mi, [&] { sv[threadIdx.x] = ov, si[threadIdx.x] = oi; });
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) done(si[0]);
}

// SpectrumPeak per frame from stored amplitude (and phase) rows: the fallback of the fused
// PEAK path for sizes / alignments the packed kernel does not take.  One workgroup per row.
template <typename T>
__global__ void __launch_bounds__(256)
peak_from_rows_kernel(const T *__restrict__ amp, const T *__restrict__ ph, int bins, T freq_scale,
                      PeakRec *__restrict__ peaks, long long batch) {
  const long long row = blockIdx.x;
  if (row >= batch) return;
  const T *a = amp + (size_t)row * (size_t)bins;
  peak_of_row(a, bins, [&](const int idx) { store_peak_from_row(peaks, row, idx, a, ph, bins, freq_scale); });
}

// findPeak per frame, spectrum.ts:74-105 (peak_of_row): the index alone.
template <typename T>
__global__ void __launch_bounds__(256)
find_peak_kernel(const T *__restrict__ amp, int bins, int *__restrict__ peak, long long batch) {
  const long long row = blockIdx.x;
  if (row >= batch) return;
  peak_of_row(amp + (size_t)row * (size_t)bins, bins, [&](const int idx) { peak[row] = idx; });
}

// Short rows (bins <= 2048): one WAVE per row, four rows per workgroup -- no LDS, no barriers, and
// a launch of `batch/4` workgroups instead of `batch` (N = 64: the workgroup-per-row form took
// 14x the time of the spectrum kernel it follows).  Same rules as find_peak_kernel /
// peak_from_rows_kernel; `ph` and `peaks` may be null / `peak` may be null (one of the outputs is set).
template <typename T>
__global__ void __launch_bounds__(256)
peak_wave_kernel(const T *__restrict__ amp, const T *__restrict__ ph, int bins, T freq_scale, int *__restrict__ peak,
                 PeakRec *__restrict__ peaks, long long batch) {
  const int lane = (int)threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
  if (row >= batch) return;
  const T *a = amp + (size_t)row * (size_t)bins;
  T bv;
  int bi;
  peak_scan<T, 64>(a, bins, lane, bv, bi);
  static_for<6>([&](auto sc) {
    constexpr int off = 32 >> sc;
    const T ov = __shfl_xor(bv, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    peak_if_wins(ov, oi, bv, bi, [&] { bv = ov, bi = oi; });
  });
  if (lane == 0) {
    if (peak) peak[row] = bi;
    if (peaks) store_peak_from_row(peaks, row, bi, a, ph, bins, freq_scale);
  }
}

}  // namespace pdsp

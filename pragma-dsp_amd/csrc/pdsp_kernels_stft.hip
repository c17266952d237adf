// Kernel unit: the complex short-time transform and its overlap-add inverse (pdsp_stft_kernel.h), f32 and f64.
// See pdsp_internal.h.  The callers in pdsp_capi_stft.hip have validated every argument.
#include "pdsp_internal.h"
#include "pdsp_stft_kernel.h"

namespace pdsp_host {

int g_istft_chunk_frames = 0;  // pdsp_set_istft_chunk_frames: 0 = the default bound below

template <typename T>
int stft_complex_dev(const pdsp_plan *plan, long long batch, const T *frames, long long frame_len,
                     long long frame_stride, const T *window, T *re_out, T *im_out, hipStream_t s) {
  const Tables<T> &t = tables<T>(plan);
  const hipError_t e = with_int<5, 13>(plan->log2n - 1, hipErrorInvalidValue, [&](auto L) {
    constexpr int LOG2M = decltype(L)::value;
    auto go = [&](auto win_c) {
      hipLaunchKernelGGL((pdsp::stft_complex_kernel<T, LOG2M, win_c>), packed_grid<LOG2M>(batch),
                         dim3(pdsp::kPackedWG<LOG2M>), 0, s, frames, window, frame_len, frame_stride, t.tw_half, t.twr,
                         re_out, im_out, batch);
      return hipGetLastError();
    };
    return window ? go(std::true_type{}) : go(std::false_type{});
  });
  PDSP_HIP_TRY(e);
  return PDSP_OK;
}

// Frames per chunk of the two-pass inverse: scratch of min(S + K, F) rows of N values, K = ceil(N / h) - 1 frames
// recomputed per chunk, S = the development switch when set, else max(K + 1, 2^28 bytes / (N sizeof T) - K) -- so
// that no chunk recomputes more frames than it finalises, and the scratch is at most
// max(256 MiB, (2K + 1) N sizeof T) whatever the number of frames F.  Also bounded so that one chunk's outputs
// (S h + N) fit a 32-bit grid.
template <typename T>
long long istft_chunk_frames(long long n, long long hop, long long frames) {
  const long long k = (n + hop - 1) / hop - 1;
  long long sf = g_istft_chunk_frames;
  if (sf <= 0) {
    sf = ((1LL << 28) / (n * (long long)sizeof(T))) - k;
    if (sf < k + 1) sf = k + 1;
  }
  const long long grid_cap = (0x7fffffffLL - 2 * n) / hop;
  if (sf > grid_cap) sf = grid_cap;
  return sf < frames ? sf : frames;
}

template <typename T>
size_t istft_scratch_bytes(long long n, long long hop, long long frames) {
  if (hop >= n) return 0;
  const long long k = (n + hop - 1) / hop - 1, rows = istft_chunk_frames<T>(n, hop, frames) + k;
  return (size_t)(rows < frames ? rows : frames) * (size_t)n * sizeof(T);
}

template <typename T>
int istft_dev(const pdsp_plan *plan, long long frames, const T *re_in, const T *im_in, long long hop, const T *window,
              T *out, hipStream_t s) {
  const Tables<T> &t = tables<T>(plan);
  const long long n = plan->n, bins = n / 2 + 1;
  const T g = T(1) / T(n);
  auto frame_launch = [&](auto direct_c, long long first, long long items, T *dst) {
    return with_int<5, 13>(plan->log2n - 1, hipErrorInvalidValue, [&](auto L) {
      constexpr int LOG2M = decltype(L)::value;
      const T *re = re_in + (size_t)first * (size_t)bins, *im = im_in + (size_t)first * (size_t)bins;
      auto go = [&](auto win_c) {
        hipLaunchKernelGGL((pdsp::istft_frame_kernel<T, LOG2M, win_c, direct_c>), packed_grid<LOG2M>(items),
                           dim3(pdsp::kPackedWG<LOG2M>), 0, s, re, im, window, first, items, frames, hop, dst,
                           t.tw_half, t.twr, g);
        return hipGetLastError();
      };
      return window ? go(std::true_type{}) : go(std::false_type{});
    });
  };
  if (hop >= n) {  // no overlap: normalise inline, one launch
    PDSP_HIP_TRY(frame_launch(std::true_type{}, 0, frames, out));
    return PDSP_OK;
  }
  const long long k = (n + hop - 1) / hop - 1;
  const long long sf = istft_chunk_frames<T>(n, hop, frames);
  const long long total = (frames - 1) * hop + n;
  StreamScratch sc(s);
  PDSP_HIP_TRY(sc.alloc(istft_scratch_bytes<T>(n, hop, frames)));
  T *const v = (T *)sc.p;
  for (long long f_lo = 0; f_lo < frames; f_lo += sf) {
    const long long f_hi = f_lo + sf < frames ? f_lo + sf : frames;
    const long long first = f_lo > k ? f_lo - k : 0;
    PDSP_HIP_TRY(frame_launch(std::false_type{}, first, f_hi - first, v));
    const long long t0 = f_lo * hop, t1 = f_hi == frames ? total : f_hi * hop;
    const long long count = t1 - t0;
    const unsigned blocks = (unsigned)((count + 255) / 256);
    if (window)
      hipLaunchKernelGGL((pdsp::istft_ola_kernel<T, true>), dim3(blocks), dim3(256), 0, s, v, window, (int)n, hop, frames,
                         first, t0, count, out);
    else
      hipLaunchKernelGGL((pdsp::istft_ola_kernel<T, false>), dim3(blocks), dim3(256), 0, s, v, window, (int)n, hop,
                         frames, first, t0, count, out);
    PDSP_HIP_TRY(hipGetLastError());
  }
  return PDSP_OK;
}

template int stft_complex_dev<float>(const pdsp_plan *, long long, const float *, long long, long long, const float *,
                                     float *, float *, hipStream_t);
template int stft_complex_dev<double>(const pdsp_plan *, long long, const double *, long long, long long, const double *,
                                      double *, double *, hipStream_t);
template int istft_dev<float>(const pdsp_plan *, long long, const float *, const float *, long long, const float *,
                              float *, hipStream_t);
template int istft_dev<double>(const pdsp_plan *, long long, const double *, const double *, long long, const double *,
                               double *, hipStream_t);
template size_t istft_scratch_bytes<float>(long long, long long, long long);
template size_t istft_scratch_bytes<double>(long long, long long, long long);

}  // namespace pdsp_host

// pdsp_capi_sdft.hip -- the sliding DFT (chosen bins at every hop): the phase tables, the handle, entry points, host form.
// Host side only; calls sdft_dev and sdft_blocks (pdsp_kernels_sdft.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <vector>

#include "pdsp_host.h"

using namespace pdsp_host;

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

namespace {

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

}  // namespace

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

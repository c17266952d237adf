// pdsp_capi_chirp.hip -- the chirp-z rows: the any-length DFT and the chirp-z transform / zoom FFT, which share ChirpTables and one host path.
// Host side only; calls dft_dev (pdsp_kernels_dft.hip) and czt_dev (pdsp_kernels_czt.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <type_traits>
#include <utility>
#include <vector>

#include "pdsp_host.h"

using namespace pdsp_host;

/* ---- chirp-z rows: the chirp-z transform, the zoom FFT and the any-length DFT ---- */

namespace {

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

}  // namespace

struct pdsp_dft : ChirpTables {};
struct pdsp_czt : ChirpTables {};

namespace {

constexpr long long kDftMinLength = 2, kDftMaxLength = 4096, kCztMaxConv = 8192;

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

}  // namespace

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

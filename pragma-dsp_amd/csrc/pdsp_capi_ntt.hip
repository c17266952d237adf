// pdsp_capi_ntt.hip -- the number-theoretic transform and exact convolution: the handle, entry points, host forms and the
// modular arithmetic of the boundary.  The only host unit that includes pdsp_goldilocks.h.
// Host side only; calls ntt_dev, ntt_blocks and ntt_mul_dev (pdsp_kernels_ntt.hip).
#include <hip/hip_runtime.h>

#include <climits>
#include <new>
#include <vector>

#include "pdsp_host.h"
#include "pdsp_goldilocks.h"

using namespace pdsp_host;

// ---- number-theoretic transform and exact convolution over GF(2^64 - 2^32 + 1) ---------------------------------
// A handle is its size and the table omega_N^j, j < N / 2, built on the host with the header the kernels compute with
// and uploaded on first use (TableHandle, first_use_table: one precision, so one slot, in the 8-byte list).

struct pdsp_ntt : TableHandle {
  long long n = 0;
  int log2n = 0;
  uint64_t *tw = nullptr;
};

namespace {

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

}  // namespace

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

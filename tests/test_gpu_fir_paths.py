"""fir_overlap_save_kernel path by path, against exact references.  The host launches one of 36 instantiations:
T in {f32, f64} x N = 64 ... 16384 x FAST in {true, false} (pdsp_kernels_fir.hip).  N sets the threads per row
(TP = N/32), the rows per workgroup (ROWS = 128 ... 1) and whether twiddles live in registers (TP >= 16).  FAST
is chosen by fir_filter_dev; _fast() below mirrors it, and every case asserts the variant it names.

References are exact: inputs and taps are integers in [-256, 256], so every output is an integer below 2^40, and
np.rint of an f64 rfft product is the exact convolution (each reference checks its own distance to the integers).
The same integers are exact in f32.  A few Gaussian cases keep realistic data, against an f64 reference of the
f32-rounded values.  Error metric: max|y - ref| / (max|x| * ||h||_2), about an rms output for white input.

The error grows with the transform's log2 N, so the bounds do too; each is 2-4x the worst error measured on an
MI355X (recorded as `worst_*` junit properties; the inputs are seeded, so the measurement repeats bit for bit):
  exact integer cases: f32 6.0e-8 ... 7.4e-8 x log2 N, bound 1.5e-7 x log2 N (worst 8.8e-7 at N = 16384);
                       f64 1.1e-16 ... 1.4e-16 x log2 N, bound 3e-16 x log2 N (worst 1.9e-15 at N = 16384);
  Gaussian cases:      f32 2.2e-8 ... 3.3e-8 x log2 N, bound 7e-8 x log2 N;
                       f64 5.3e-17 ... 6.6e-17 x log2 N, bound 1.6e-16 x log2 N.
Frequency response, per component against a long-double DFT: f32 within 1 ulp + 2^-40 * sum|h|, measured 0.4996
of that bound (the kernel sums in f64 and rounds once: correctly rounded); f64 within SPEC_TOL_F64[N] * sum|h|,
about 4x the worst measured (5.7e-17 at N = 64 falling to 9.5e-18 at N = 16384).
FAST and clamped differ only in loads and stores, so the invariances below are bitwise."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NS = [64 << i for i in range(9)]  # 64 ... 16384
TOL = {"f32": 1.5e-7, "f64": 3e-16}        # x log2 N, exact integer references
TOL_GAUSS = {"f32": 7e-8, "f64": 1.6e-16}  # x log2 N, Gaussian data
SPEC_TOL_F64 = {64: 2.2e-16, 128: 1.5e-16, 256: 1.5e-16, 512: 1.1e-16, 1024: 9e-17, 2048: 6.5e-17, 4096: 7e-17,
                8192: 4.5e-17, 16384: 3.8e-17}
SENTINEL = -12345.0
MODES = ("full", "same", "valid", "filter")


@pytest.fixture(scope="module")
def pd():
    import pragma_dsp_amd
    return pragma_dsp_amd


def tol(dt, n, table=TOL):
    return table[dt] * (n.bit_length() - 1)


def _t(key):
    import torch
    return torch.float32 if key == "f32" else torch.float64


def _geom(n, ntaps):
    """(p1, hop) of the launch: an even filter runs with one zero tap more, so p1 = P - 1 for odd P, P for even P."""
    p1 = ntaps - 1 if ntaps % 2 else ntaps
    return p1, n - p1


def _rows_per_wg(n):
    tp = n // 32
    return max(tp, 256) // tp


def _fast(x_ptr, y_ptr, x_stride, y_stride, n, ntaps, y_off):
    """Mirror of fir_filter_dev's `fast`: 8-byte aligned x and y, even strides, even hop, even y_off - p1."""
    p1, hop = _geom(n, ntaps)
    return ((x_ptr | y_ptr) & 7) == 0 and x_stride % 2 == 0 and y_stride % 2 == 0 and hop % 2 == 0 \
        and (y_off - p1) % 2 == 0


def _ints(rng, shape):
    return rng.integers(-256, 257, size=shape).astype(np.float64)


def _taps(rng, p):
    h = _ints(rng, p)
    h[0] = h[0] or 1.0
    return h


def exact_full(x, h):
    """Exact full convolution of integer rows x [rows, len] with integer taps h."""
    n = x.shape[-1] + h.size - 1
    nfft = 1 << max(n - 1, 0).bit_length()
    r = np.fft.irfft(np.fft.rfft(x, nfft) * np.fft.rfft(h, nfft), nfft)[..., :n]
    q = np.rint(r)
    assert np.abs(r - q).max() < 0.05  # the f64 product is close enough that rint is exact
    return q


def f64_full(x, h):
    n = x.shape[-1] + h.size - 1
    if x.shape[-1] * h.size <= 1 << 20:
        return np.stack([np.convolve(r, h) for r in x])
    nfft = 1 << (n - 1).bit_length()
    return np.fft.irfft(np.fft.rfft(x, nfft) * np.fft.rfft(h, nfft), nfft)[..., :n]


def err(y, want, x, h):
    return float(np.abs(y.astype(np.float64) - want).max() / (max(np.abs(x).max(), 1.0) * np.linalg.norm(h)))


class Buf:
    """rows of `length` at `stride`, starting `off` elements into a buffer with `guard` elements after the last
    row; everything outside the rows holds `fill`."""

    def __init__(self, dtype, rows, length, stride, off, fill, guard=64):
        import torch
        self.rows, self.length, self.stride, self.off = rows, length, stride, off
        self.flat = torch.full((off + (rows - 1) * stride + length + guard,), fill, dtype=dtype, device="cuda:0")
        self.view = torch.as_strided(self.flat, (rows, length), (stride, 1), off)
        self.ptr = self.view.data_ptr()

    def outside(self):
        """Every element of the buffer that is not in a row."""
        mask = np.ones(self.flat.numel(), bool)
        idx = self.off + np.arange(self.rows)[:, None] * self.stride + np.arange(self.length)[None, :]
        mask[idx.reshape(-1)] = False
        return self.flat.cpu().numpy()[mask]


def _layout(dtype, rows, length, y_len, fast):
    """(x Buf, y Buf) for the named variant.  FAST: even offsets, even strides.  Clamped: odd offsets (4-byte
    alignment in f32) and odd strides (f64, whose every element is 8-byte aligned).  The input's gaps and guards
    hold NaN, so a load outside a row cannot go unseen; the output's hold SENTINEL."""
    if fast:
        xs, ys, xo, yo = length + 2 + length % 2, y_len + 2 + y_len % 2, 2, 4
    else:
        xs, ys, xo, yo = length + 1 + length % 2, y_len + 3, 1, 3
    return Buf(dtype, rows, length, xs, xo, float("nan")), Buf(dtype, rows, y_len, ys, yo, SENTINEL)


def _raw(pd, f, xb, length, y_off, y_len, yb, rows=None, x_ptr=None, x_stride=None):
    """pdsp_fir_filter_* on explicit pointers and strides, on the stream f was built on; returns the status."""
    import torch
    from pragma_dsp_amd._capi import lib
    fn = getattr(lib, f"pdsp_fir_filter_{f._sfx}")
    return fn(f.plan._h, xb.rows if rows is None else rows, C.c_void_p(xb.ptr if x_ptr is None else x_ptr), length,
              xb.stride if x_stride is None else x_stride, C.c_void_p(f.h_re.data_ptr()),
              C.c_void_p(f.h_im.data_ptr()), f.ntaps, y_off, y_len, C.c_void_p(yb.ptr), yb.stride,
              C.c_void_p(torch.cuda.current_stream().cuda_stream))


def run_case(pd, f, x, mode, fast):
    """Filter the rows x [rows, len] through the named variant; returns (y [rows, y_len], y_off).  Asserts the
    variant by the mirror and that nothing outside the output rows changed."""
    import torch
    from pragma_dsp_amd.filters import output_range
    rows, length = x.shape
    y_off, y_len = output_range(length, f.ntaps, mode)
    xb, yb = _layout(f.dtype, rows, length, y_len, fast)
    xb.view.copy_(torch.from_numpy(x).to(f.dtype))
    assert _fast(xb.ptr, yb.ptr, xb.stride, yb.stride, f.size, f.ntaps, y_off) == fast, (mode, rows, length)
    assert _raw(pd, f, xb, length, y_off, y_len, yb) == 0
    torch.cuda.synchronize()
    assert (yb.outside() == SENTINEL).all(), "write outside the output rows"
    return yb.view.cpu().numpy(), y_off


def _matrix(n):
    """(ntaps, mode, rows, len, fast) cases for one N: several blocks per row with both output parities, every mode
    at len < P, len = P and len = 1, and rows x blocks = k ROWS - 1, k ROWS, k ROWS + 1 (dead rows in the last
    workgroup), once as rows of one block and once as one row of many blocks."""
    rw = _rows_per_wg(n)
    out = []
    for p in sorted({1, 2, 5, n // 2 - 1, n // 2}):
        p1, hop = _geom(n, p)
        long_ = 3 * hop + n + 2  # interior blocks lie wholly inside the row
        for mode in MODES:
            for length in (long_, long_ + 1):
                off = {"full": 0, "same": (p - 1) // 2, "valid": p - 1, "filter": 0}[mode]
                for fast in ((True, False) if (off - p1) % 2 == 0 else (False,)):
                    out.append((p, mode, 3, length, fast))
        for length in sorted({1, max(p // 2, 1), p}):
            for mode in MODES:
                off = {"full": 0, "same": (min(length, p) - 1) // 2, "valid": min(length, p) - 1, "filter": 0}[mode]
                for fast in ((True, False) if (off - p1) % 2 == 0 else (False,)):
                    out.append((p, mode, 2, length, fast))
        if p in (1, n // 2):
            for items in (2 * rw - 1, 2 * rw, 2 * rw + 1):
                if items < 1:
                    continue
                out.append((p, "filter", items, hop - 1, False))      # one block per row
                out.append((p, "filter", items, hop, True))
                out.append((p, "filter", 1, (items - 1) * hop + 2, True))  # one row of `items` blocks
    return out


def _nblk(n, p, mode, length):
    from pragma_dsp_amd.filters import output_range
    return -(-output_range(length, p, mode)[1] // _geom(n, p)[1])


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", NS)
def test_instantiation_matrix(pd, record_property, dt, n):
    """Every (T, N) through both FAST and clamped, exact integer references, guard bands around every output."""
    rng = np.random.default_rng(n * 2 + (dt == "f64"))
    worst, seen, filters = 0.0, set(), {}
    for p, mode, rows, length, fast in _matrix(n):
        if p not in filters:
            h = _taps(rng, p)
            filters[p] = (h, pd.FirFilter(h, "cuda:0", _t(dt), block=n))
        h, f = filters[p]
        x = _ints(rng, (rows, length))
        y, off = run_case(pd, f, x, mode, fast)
        want = exact_full(x, h)[:, off:off + y.shape[1]]
        e = err(y, want, x, h)
        worst = max(worst, e)
        seen.add(fast)
        assert e <= tol(dt, n), (n, p, mode, rows, length, fast, e)
    record_property("worst_err", worst)
    assert seen == {True, False}
    # the rows x blocks counts reached the dead rows of a last workgroup
    rw = _rows_per_wg(n)
    if rw > 1:
        assert any(r * _nblk(n, p, m, ln) % rw for p, m, r, ln, _ in _matrix(n))


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", [64, 1024, 16384])
def test_gaussian_against_f64(pd, record_property, dt, n):
    """Realistic data: Gaussian rows and taps, the reference in f64 on the values the kernel sees."""
    rng = np.random.default_rng(100 + n)
    worst = 0.0
    for p in (3, n // 2):
        h = rng.standard_normal(p)
        f = pd.FirFilter(h, "cuda:0", _t(dt), block=n)
        hq = h.astype(np.float32).astype(np.float64) if dt == "f32" else h
        for fast in (True, False):
            x = rng.standard_normal((2, 4 * n + 2 + (not fast)))
            xq = x.astype(np.float32).astype(np.float64) if dt == "f32" else x
            y, off = run_case(pd, f, x, "full", fast)
            e = err(y, f64_full(xq, hq), xq, hq)
            worst = max(worst, e)
            assert e <= tol(dt, n, TOL_GAUSS), (n, p, fast, e)
    record_property("worst_err", worst)


# ---- the filter spectrum to the rounding ------------------------------------------------------------------------

_PI_L = np.longdouble("3.14159265358979323846264338327950288")


def exact_dft(h, n):
    """H[k] = sum_j h[j] e^{-2 pi i j k / n}, k = 0 ... n/2, in long double with reduced arguments (j k) mod n."""
    m = np.arange(n, dtype=np.longdouble)
    ang = 2 * _PI_L * m / np.longdouble(n)
    c, s = np.cos(ang), np.sin(ang)
    hl = h.astype(np.longdouble)
    j = np.arange(h.size, dtype=np.int64)
    k = np.arange(n // 2 + 1, dtype=np.int64)
    re = np.empty(k.size, np.longdouble)
    im = np.empty(k.size, np.longdouble)
    step = max(1, (1 << 21) // h.size)
    for a in range(0, k.size, step):
        idx = (k[a:a + step, None] * j[None, :]) % n
        re[a:a + step] = (c[idx] * hl).sum(axis=1)
        im[a:a + step] = -(s[idx] * hl).sum(axis=1)
    return re, im


@pytest.mark.parametrize("n", NS)
def test_frequency_response_to_the_rounding(pd, record_property, n):
    """Every bin, each component: f32 within 1 ulp + 2^-40 sum|h| of the exact value, f64 within SPEC_TOL_F64[N] *
    sum|h|.  An f32-accumulated spectrum is many ulps off at P = N/2."""
    import torch
    rng = np.random.default_rng(7 * n)
    worst32, worst64 = 0.0, 0.0
    for p in (1, n // 2):
        h = rng.standard_normal(p).astype(np.float32).astype(np.float64)  # the same values in both precisions
        ere, eim = exact_dft(h, n)
        l1 = np.abs(h).sum()
        for dt in ("f32", "f64"):
            f = pd.FirFilter(h, "cuda:0", _t(dt), block=n)
            gre, gim = (t.cpu().numpy() for t in f.frequency_response())
            assert gre.shape == gim.shape == (n // 2 + 1,)
            for got, ex in ((gre, ere), (gim, eim)):
                d = np.abs(got.astype(np.longdouble) - ex).astype(np.float64)
                if dt == "f32":
                    ulp = np.spacing(np.abs(ex.astype(np.float64)).astype(np.float32)).astype(np.float64)
                    worst32 = max(worst32, float((d / (ulp + 2.0 ** -40 * l1)).max()))
                    assert (d <= ulp + 2.0 ** -40 * l1).all(), (n, p, np.argmax(d - ulp))
                else:
                    worst64 = max(worst64, float(d.max() / l1))
                    assert d.max() <= SPEC_TOL_F64[n] * l1, (n, p, d.max() / l1)
    record_property("worst_f32_in_ulp_bound", worst32)
    record_property("worst_f64_rel_l1", worst64)


# ---- exact invariances ------------------------------------------------------------------------------------------

def _filter_rows(pd, f, x, y_off, y_len, fast, length=None):
    """Raw call on rows x [rows, len] (optionally with `length` < len: the rest is explicit padding in memory)."""
    import torch
    rows, xl = x.shape
    xb, yb = _layout(f.dtype, rows, xl, y_len, fast)
    xb.view.copy_(torch.from_numpy(x).to(f.dtype))
    assert _fast(xb.ptr, yb.ptr, xb.stride, yb.stride, f.size, f.ntaps, y_off) == fast
    assert _raw(pd, f, xb, xl if length is None else length, y_off, y_len, yb) == 0
    torch.cuda.synchronize()
    return yb.view.cpu().numpy()


INV = [("f32", 64, 5), ("f32", 4096, 2047), ("f32", 16384, 8192), ("f64", 256, 128), ("f64", 4096, 301),
       ("f64", 16384, 8191)]


@pytest.mark.parametrize("dt,n,p", INV)
def test_row_position_and_block_shift(pd, dt, n, p):
    """A row gives the same bits alone and at row 37 of a batch; hop leading zeros shift the output by hop."""
    rng = np.random.default_rng(n + p)
    h = _taps(rng, p)
    f = pd.FirFilter(h, "cuda:0", _t(dt), block=n)
    p1, hop = _geom(n, p)
    for fast in (True, False):
        length = 3 * hop + n + 2 + (not fast)
        x = _ints(rng, (50, length))
        y_len = length + p - 1
        batch = _filter_rows(pd, f, x, 0, y_len, fast)
        alone = _filter_rows(pd, f, x[37:38], 0, y_len, fast)
        assert np.array_equal(alone[0], batch[37])
        xs = np.concatenate([np.zeros((1, hop)), x[37:38]], axis=1)
        shifted = _filter_rows(pd, f, xs, 0, y_len + hop, fast)
        assert np.array_equal(shifted[0, hop:], batch[37])
        assert np.array_equal(shifted[0, :hop], np.zeros(hop))


@pytest.mark.parametrize("dt,n,p", INV)
def test_padding_and_variant_independence(pd, dt, n, p):
    """Zeros in memory past len give the bits of the clamped loads' implicit zeros; FAST and clamped agree."""
    rng = np.random.default_rng(3 * n + p)
    h = _taps(rng, p)
    f = pd.FirFilter(h, "cuda:0", _t(dt), block=n)
    p1, hop = _geom(n, p)
    length = 4 * hop + 6
    x = _ints(rng, (3, length))
    y_len = length + p - 1
    for fast in (True, False):
        ref = _filter_rows(pd, f, x, 0, y_len, fast)
        padded = np.concatenate([x, np.zeros((3, n + 2))], axis=1)
        got = _filter_rows(pd, f, padded, 0, y_len, fast, length=length + n + 2)
        assert np.array_equal(got, ref), fast
    for mode_off in (0, p1 // 2 * 2):  # full and an even offset into it
        a = _filter_rows(pd, f, x, mode_off, y_len - mode_off, True)
        b = _filter_rows(pd, f, x, mode_off, y_len - mode_off, False)
        assert np.array_equal(a, b), mode_off


@pytest.mark.parametrize("dt,n,p", INV)
def test_power_of_two_scaling(pd, dt, n, p):
    """y(x 2^k) == y(x) 2^k bit for bit.  k = +-60 in f32 and +-900 in f64 keep every intermediate of these
    integer inputs (at most 2^8 in, 2^44 inside the transforms) normal and finite."""
    rng = np.random.default_rng(5 * n + p)
    h = _taps(rng, p)
    f = pd.FirFilter(h, "cuda:0", _t(dt), block=n)
    p1, hop = _geom(n, p)
    x = _ints(rng, (2, 3 * hop + n + 2))
    y_len = x.shape[1] + p - 1
    for fast in (True, False):
        base = _filter_rows(pd, f, x, 0, y_len, fast)
        for k in ((60, -60) if dt == "f32" else (900, -900)):
            got = _filter_rows(pd, f, np.ldexp(x, k), 0, y_len, fast)
            assert np.array_equal(got, np.ldexp(base.astype(np.float64), k).astype(base.dtype)), (fast, k)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", [64, 4096])
def test_row_isolation(pd, dt, n):
    """NaN in one row and +-Inf in another: every other row keeps its bits, and so do the blocks of the affected
    rows that do not read the bad sample.  At N = 64 128 rows share a workgroup."""
    rng = np.random.default_rng(n + 99)
    p = n // 4 + 1
    h = _taps(rng, p)
    f = pd.FirFilter(h, "cuda:0", _t(dt), block=n)
    p1, hop = _geom(n, p)
    rows, length = 300 if n == 64 else 6, 6 * hop + 7
    x = _ints(rng, (rows, length))
    y_len = length + p - 1
    for fast in (True, False):
        clean = _filter_rows(pd, f, x, 0, y_len, fast)
        bad = x.copy()
        hits = {5: [(2 * hop + 3, np.nan)], 130 % rows: [(hop + 1, np.inf), (4 * hop + 10, -np.inf)]}
        for r, pts in hits.items():
            for t, v in pts:
                bad[r, t] = v
        dirty = _filter_rows(pd, f, bad, 0, y_len, fast)
        keep = np.ones(rows, bool)
        keep[list(hits)] = False
        assert np.array_equal(dirty[keep], clean[keep]), fast
        for r, pts in hits.items():
            ok = np.ones(y_len, bool)
            for t, _ in pts:
                for b in range(-(-y_len // hop)):
                    s = b * hop - p1
                    if s <= t < s + n:
                        ok[b * hop:(b + 1) * hop] = False
            assert ok.any() and not ok.all()
            assert np.array_equal(dirty[r, ok], clean[r, ok]), (fast, r)
            assert not np.isfinite(dirty[r, ~ok]).all()


# ---- aliasing and stream ordering -------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_output_overlapping_input_is_refused(pd, dt):
    """out = x and a partly overlapping out are refused before any launch, through Python and through the C ABI;
    an out that touches x but shares no byte still works."""
    import torch
    from pragma_dsp_amd import _capi
    rng = np.random.default_rng(17)
    h = _taps(rng, 33)
    f = pd.FirFilter(h, "cuda:0", _t(dt), block=256)
    length = 3000
    x = _ints(rng, length)
    want = exact_full(x[None], h)[0, :length]
    buf = torch.full((2 * length + 8,), SENTINEL, dtype=_t(dt), device="cuda:0")
    buf[:length] = torch.from_numpy(x).to(_t(dt))
    xv = buf[:length]
    for out in (xv, buf[length - 5:2 * length - 5], buf[1:length + 1]):
        before = buf.cpu().numpy()
        with pytest.raises(pd.PdspError, match="overlaps input") as e:
            f.apply(xv, "filter", out=out)
        assert e.value.code == _capi.ERR_BAD_ARG
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), before, equal_nan=True)
    # C ABI, strided rows: y starts inside the last input row, or right behind it (the buffer holds that y too)
    xb = Buf(_t(dt), 4, 500, 512, 0, 0.0, guard=4 * 512)
    yb = Buf(_t(dt), 4, 500, 512, 0, SENTINEL)
    for y_ptr, ok in ((xb.ptr, False), (xb.ptr + (3 * 512 + 499) * xb.flat.element_size(), False),
                      (xb.ptr + (3 * 512 + 500) * xb.flat.element_size(), True)):
        yb.ptr = y_ptr
        rc = _raw(pd, f, xb, 500, 0, 500, yb)
        if ok:
            assert rc == 0
        else:
            assert rc == _capi.ERR_BAD_ARG and b"overlaps input" in _capi.lib.pdsp_last_error()
    torch.cuda.synchronize()
    # touching but disjoint: y right behind x in the same buffer
    y = f.apply(xv, "filter", out=buf[length:2 * length])
    torch.cuda.synchronize()
    assert y.data_ptr() == xv.data_ptr() + length * buf.element_size()
    assert err(y.cpu().numpy(), want, x, h) <= tol(dt, 256)
    assert np.array_equal(buf[:length].cpu().numpy(), x.astype(np.float32 if dt == "f32" else np.float64))


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_spectrum_ordered_before_another_stream(pd, monkeypatch, dt):
    """The filter spectrum is written on the stream current at construction; apply() and frequency_response() on a
    new non-blocking stream must wait for it.  Constructing uploads the taps synchronously, so a sleep queued before
    the constructor would be over by the spectrum launch: the sleep goes onto the construction stream right in front
    of pdsp_fir_spectrum_*, through a wrapper around the library."""
    import torch
    import pragma_dsp_amd.filters as F
    real = F.lib

    class Held:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith("pdsp_fir_spectrum_"):
                return fn

            def held(*a):
                torch.cuda._sleep(50_000_000)  # tens of milliseconds or more on the current stream
                return fn(*a)
            return held

    rng = np.random.default_rng(23)
    h = _taps(rng, 8191)
    x = _ints(rng, (2, 40000))
    xt = torch.from_numpy(x).to(_t(dt)).cuda()
    want = exact_full(x, h)
    torch.cuda.synchronize()
    monkeypatch.setattr(F, "lib", Held())
    f = pd.FirFilter(h, "cuda:0", _t(dt), block=16384)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        y = f.apply(xt, "full")
    g = pd.FirFilter(h, "cuda:0", _t(dt), block=16384)
    with torch.cuda.stream(side):
        hre = g.frequency_response()[0].clone()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert err(y.cpu().numpy(), want, x, h) <= tol(dt, 16384)
    assert np.array_equal(hre.cpu().numpy(), f.h_re.cpu().numpy())

"""hilbert / hilbert_imag / envelope / instantaneous_phase on the device (pdsp_hilbert_kernel.h): every
N = 64 ... 16384 x f32 / f64 x four output modes x both kernel paths against the f64 numpy restatement of
test_hilbert_cpu (itself pinned to scipy.signal.hilbert there), computed from the same inputs rounded to the dtype.

Metric per row, a_ref the reference analytic signal: max|out - ref| / max|a_ref| for the analytic signal, its
imaginary part and the envelope; max over samples of |wrap(phi - phi_ref)| |a_ref| / max|a_ref| for the phase, so that
no sample is excluded and a phase is asked as exactly as its sample is large.

Bound: the computation is the forward-split / inverse-split round trip that istft(stft(x)) makes, with an exact
multiplication by -i in between, so it is that round trip's own bound, RT_TOL of test_gpu_stft_pair.py (1e-7 in f32,
1.6e-16 in f64) times log2 N; the phase gets 4 eps(T) on top (two ulp of a value in [2, 4)) for the atan2 itself.

Both kernel paths are reached on purpose: FAST (_fast() mirrors hilbert_fast_path in pdsp_kernels_hilbert.hip) and the
general one (a one-element offset, odd strides, len < N).  They differ only in how rows move, so their results are
bitwise equal, and so are in place vs out of place, repeated calls and the host f64 form vs BatchedFft f64."""
import ctypes as C

import numpy as np
import pytest

from test_hilbert_cpu import MODES, NS, hilbert_ref, mode_ref

pytestmark = pytest.mark.gpu

RT_TOL = {"f32": 1e-7, "f64": 1.6e-16}  # x log2 N (tests/test_gpu_stft_pair.py)
EPS = {"f32": 2.0 ** -23, "f64": 2.0 ** -52}
SENTINEL = float("nan")


def bound(dt, n, mode):
    return RT_TOL[dt] * (n.bit_length() - 1) + (4 * EPS[dt] if mode == "phase" else 0.0)


@pytest.fixture(scope="module")
def pd():
    import pragma_dsp_amd
    return pragma_dsp_amd


def _t(key):
    import torch
    return torch.float32 if key == "f32" else torch.float64


_plans = {}


def plan(pd, n, dt):
    from pragma_dsp_amd.batch import BatchedFft
    key = (n, dt)
    if key not in _plans:
        _plans[key] = BatchedFft(n, dtype=_t(dt))
    return _plans[key]


def rows_per_wg(n):
    tp = n // 32
    return max(tp, 256) // tp


def run(p, x, mode, out=None):
    return {"analytic": p.hilbert, "imag": p.hilbert_imag, "envelope": p.envelope,
            "phase": p.instantaneous_phase}[mode](x, out=out)


def _fast(p, x, y, mode):
    """Mirror of hilbert_fast_path: len == N, x rows aligned to 2 elements with an even stride, y rows aligned to 2
    elements (analytic: to 16 bytes) with a stride that keeps that."""
    es = x.element_size()
    rows, ln = x.shape
    k = 2 if mode == "analytic" else 1
    xs = x.stride(0) if rows > 1 else p.size
    ys = k * y.stride(0) if rows > 1 else k * p.size
    ya = 16 if mode == "analytic" else 2 * es
    return (ln == p.size and x.data_ptr() % (2 * es) == 0 and xs % 2 == 0 and y.data_ptr() % ya == 0
            and (ys * es) % ya == 0)


def to_np(y):
    return y.cpu().numpy()


def err_rows(got, a_ref, mode):
    """The metric of the module docstring, its maximum over the rows."""
    got = np.asarray(got, np.complex128 if mode == "analytic" else np.float64)
    den = np.abs(a_ref).max(axis=-1, keepdims=True)
    den = np.where(den > 0, den, 1.0)
    if mode == "phase":
        dphi = np.angle(np.exp(1j * (got - np.angle(a_ref))))
        return (np.abs(dphi) * np.abs(a_ref) / den).max()
    return (np.abs(got - mode_ref(a_ref, mode)) / den).max()


def strided(rows, n, stride, dt, offset=0, fill=SENTINEL, cplx=False):
    """A [rows, n] view at row stride `stride`, `offset` elements into a buffer filled with `fill`."""
    import torch
    t = _t(dt)
    if cplx:
        t = torch.complex64 if dt == "f32" else torch.complex128
    buf = torch.full((offset + rows * stride + 8,), fill, dtype=t, device="cuda")
    return buf, buf.as_strided((rows, n), (stride, 1), offset)


def normal_rows(seed, rows, n, dt):
    import torch
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((rows, n))).to(_t(dt)).cuda()


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", NS)
def test_every_mode_and_path_against_numpy(pd, n, dt):
    import torch
    p = plan(pd, n, dt)
    rows = 5
    x = normal_rows(n + (dt == "f64"), rows, n, dt)
    a_ref = hilbert_ref(x.double().cpu().numpy())
    # general path three ways: a one-element offset, an odd stride, len < N
    _, xo = strided(rows, n, n, dt, offset=1)
    xo.copy_(x)
    _, xs = strided(rows, n, n + 1, dt)
    xs.copy_(x)
    ln = n - 3
    xl = x[:, :ln]
    a_len = hilbert_ref(xl.double().cpu().numpy(), n)
    for mode in MODES:
        y = run(p, x, mode)
        assert _fast(p, x, y, mode)
        e = err_rows(to_np(y), a_ref, mode)
        print(f"HILBERR {dt} n={n} {mode} fast {e:.3e} bound {bound(dt, n, mode):.3e}")
        assert e <= bound(dt, n, mode), (n, dt, mode, "fast", e)
        for name, xin, ref in (("offset", xo, a_ref), ("stride", xs, a_ref), ("len", xl, a_len)):
            y = run(p, xin, mode)
            assert not _fast(p, xin, y, mode), name
            e = err_rows(to_np(y), ref, mode)
            print(f"HILBERR {dt} n={n} {mode} {name} {e:.3e} bound {bound(dt, n, mode):.3e}")
            assert e <= bound(dt, n, mode), (n, dt, mode, name, e)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", NS)
def test_real_half_is_the_input_bit_for_bit(pd, n, dt):
    import torch
    p = plan(pd, n, dt)
    x = normal_rows(3 * n, 4, n, dt)
    a = p.hilbert(x)
    assert a.dtype == (torch.complex64 if dt == "f32" else torch.complex128) and tuple(a.shape) == (4, n)
    ib = torch.int32 if dt == "f32" else torch.int64
    assert torch.equal(torch.view_as_real(a)[..., 0].contiguous().view(ib), x.view(ib))
    _, xs = strided(4, n, n + 1, dt)  # general path
    xs.copy_(x)
    a2 = p.hilbert(xs)
    assert torch.equal(torch.view_as_real(a2).view(ib), torch.view_as_real(a).view(ib))
    # padded: the real half is x, then zeros
    a3 = torch.view_as_real(p.hilbert(x[:, :n // 2]))[..., 0]
    assert torch.equal(a3[:, :n // 2].contiguous().view(ib), x[:, :n // 2].contiguous().view(ib))
    assert torch.equal(a3[:, n // 2:], torch.zeros_like(a3[:, n // 2:]))


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", NS)
def test_paths_in_place_and_repeats_are_bitwise(pd, n, dt):
    import torch
    p = plan(pd, n, dt)
    rows = 3
    xc = normal_rows(n, rows, n, dt)
    es = xc.element_size()
    for mode in MODES:
        cplx = mode == "analytic"
        ref = run(p, xc, mode)
        assert _fast(p, xc, ref, mode)
        assert torch.equal(run(p, xc, mode), ref)  # repeated call
        # general path: a one-element offset (misaligned rows) ...
        _, xo = strided(rows, n, n, dt, offset=1)
        xo.copy_(xc)
        yo = run(p, xo, mode)
        assert not _fast(p, xo, yo, mode)
        assert torch.equal(yo, ref)
        # ... odd strides on both sides
        _, xs = strided(rows, n, n + 1, dt)
        xs.copy_(xc)
        _, ys = strided(rows, n, n + 3, dt, cplx=cplx)
        run(p, xs, mode, out=ys)
        assert not _fast(p, xs, ys, mode)
        assert torch.equal(ys, ref)
        # FAST with padded strides (multiples of 16 bytes)
        pad = 16 // es
        _, xf = strided(rows, n, n + pad, dt)
        xf.copy_(xc)
        _, yf = strided(rows, n, n + 2 * pad, dt, cplx=cplx)
        run(p, xf, mode, out=yf)
        assert _fast(p, xf, yf, mode)
        assert torch.equal(yf, ref)
        if cplx:
            continue
        # exact in place, on both paths
        xi = xc.clone()
        assert run(p, xi, mode, out=xi).data_ptr() == xi.data_ptr()
        assert torch.equal(xi, ref)
        run(p, xs, mode, out=xs)
        assert torch.equal(xs, ref)
        # in place with len < N: x is the first len samples of the rows that receive the N outputs
        ln = n - 3
        want = run(p, xc[:, :ln], mode)
        for stride in (n, n + 1):
            _, yi = strided(rows, n, stride, dt)
            yi[:, :ln].copy_(xc[:, :ln])
            got = run(p, yi[:, :ln], mode, out=yi)
            assert got.data_ptr() == yi.data_ptr()
            assert torch.equal(yi, want), stride


@pytest.mark.parametrize("n", [64, 1024, 16384])
def test_host_form_matches_device_f64_bitwise(pd, n):
    import torch
    p = plan(pd, n, "f64")
    x = np.random.default_rng(5).standard_normal((4, n))
    xd = torch.from_numpy(x).cuda()
    for ln in (n, n // 2 + 1):
        a = pd.hilbert(x[:, :ln], n)
        assert a.dtype == np.complex128 and a.shape == (4, n)
        assert np.array_equal(a, to_np(p.hilbert(xd[:, :ln])))
        assert np.array_equal(pd.envelope(x[:, :ln], n), to_np(p.envelope(xd[:, :ln])))
        assert np.array_equal(pd.instantaneous_phase(x[:, :ln], n), to_np(p.instantaneous_phase(xd[:, :ln])))
    # 1-D input, n defaulted to the row length
    assert np.array_equal(pd.hilbert(x[1]), to_np(p.hilbert(xd[1:2]))[0])
    assert np.array_equal(pd.envelope(x[2]), to_np(p.envelope(xd[2:3]))[0])
    assert np.array_equal(pd.instantaneous_phase(x[3]), to_np(p.instantaneous_phase(xd[3:4]))[0])


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", [64, 2048, 16384])
def test_exact_cases(pd, n, dt):
    import torch
    p = plan(pd, n, dt)
    nn = np.arange(n)
    ks = [1, 5, n // 4, n // 2 - 1]
    # the angle reduced exactly (integer phase mod N) so that the inputs are correct to the last bit
    ph = np.stack([2 * np.pi * ((k * nn) % n) / n for k in ks])
    x = torch.from_numpy(np.cos(ph)).to(_t(dt)).cuda()
    # the reference is hilbert_ref of the inputs as rounded to the dtype, like everywhere else in this file; those
    # inputs are cosines to within eps(T) / 2 a sample, and the Hilbert transform of such noise is at most
    # (2 / pi) ln N + 2 times as large in the maximum norm (the l1 norm of its kernel), which is below 2 log2 N: so
    # the reference itself is the sine, and its envelope 1, to within eps(T) log2 N
    xh = x.double().cpu().numpy()
    a_ref = hilbert_ref(xh)
    own = EPS[dt] * (n.bit_length() - 1)
    assert np.abs(a_ref.imag - np.sin(ph)).max() <= own and np.abs(np.abs(a_ref) - 1).max() <= own
    b = bound(dt, n, "imag")
    h = to_np(p.hilbert_imag(x)).astype(np.float64)
    assert np.abs(h - a_ref.imag).max() <= b, np.abs(h - a_ref.imag).max()
    env = to_np(p.envelope(x)).astype(np.float64)
    assert np.abs(env - np.abs(a_ref)).max() <= b, np.abs(env - np.abs(a_ref)).max()
    # a constant row and the Nyquist row: DC and Nyquist are written as zeros and every other bin of such a row is an
    # exact zero of the butterflies, so Hx == 0 exactly
    flat = np.stack([np.full(n, 0.75), np.full(n, -3.0), (-1.0) ** nn, -0.3 * (-1.0) ** nn])
    xf = torch.from_numpy(flat).to(_t(dt)).cuda()
    h = to_np(p.hilbert_imag(xf)).astype(np.float64)
    if np.any(h != 0):
        spec = np.abs(np.fft.rfft(h, axis=-1))
        bins = sorted({int(k) for r in range(h.shape[0]) for k in np.nonzero(spec[r] > 0)[0]})
        raise AssertionError(f"Hx of a constant / Nyquist row is not exactly zero: max|Hx| = {np.abs(h).max():.3e}, "
                             f"non-zero bins of Hx (first 16): {bins[:16]}")
    env = to_np(p.envelope(xf))
    want = np.abs(to_np(xf))
    assert np.abs(env.astype(np.float64) - want).max() <= np.spacing(want.astype(env.dtype)).max()  # 1 ulp


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", [64, 1024, 16384])
def test_padding(pd, n, dt):
    p = plan(pd, n, dt)
    x = normal_rows(9, 3, n, dt)
    for ln in (1, n // 2, n - 1):
        xl = x[:, :ln]
        a_ref = hilbert_ref(xl.double().cpu().numpy(), n)
        for mode in MODES:
            y = run(p, xl, mode)
            assert tuple(y.shape) == (3, n)
            e = err_rows(to_np(y), a_ref, mode)
            assert e <= bound(dt, n, mode), (n, dt, mode, ln, e)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", [64, 256, 2048, 16384])
def test_guard_bands(pd, n, dt):
    import torch
    p = plan(pd, n, dt)
    rows = 4
    xc = normal_rows(2, rows, n, dt)
    es = xc.element_size()
    for mode in MODES:
        cplx = mode == "analytic"
        k = 2 if cplx else 1
        ref = run(p, xc, mode)
        for xpad, ypad, off, ln in ((16 // es, 16 // es, 0, n), (3, 5, 1, n), (3, 5, 1, n - 5)):
            if ln != n:
                ref_l = run(p, xc[:, :ln].contiguous(), mode)
            _, xs = strided(rows, ln, n + xpad, dt)  # NaN in the stride gaps of x (and behind len)
            xs.copy_(xc[:, :ln])
            ybuf, ys = strided(rows, n, n + ypad, dt, offset=off, cplx=cplx)  # NaN sentinels around and between rows
            before = ybuf.clone()
            run(p, xs, mode, out=ys)
            assert torch.equal(ys, ref if ln == n else ref_l)
            yr = torch.view_as_real(ybuf).reshape(-1) if cplx else ybuf
            br = torch.view_as_real(before).reshape(-1) if cplx else before
            mask = torch.ones_like(yr, dtype=torch.bool)
            for r in range(rows):
                mask[k * (off + r * (n + ypad)): k * (off + r * (n + ypad) + n)] = False
            ib = torch.int32 if dt == "f32" else torch.int64
            assert torch.equal(yr.view(ib)[mask], br.view(ib)[mask])  # bitwise: gaps and bands untouched


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", NS)
def test_batches_with_dead_rows(pd, n, dt):
    p = plan(pd, n, dt)
    R = rows_per_wg(n)
    for rows in sorted({1, R - 1, R + 1, 67} - {0}):
        x = normal_rows(rows, rows, n, dt)
        a_ref = hilbert_ref(x.double().cpu().numpy())
        for mode in ("analytic", "envelope"):
            e = err_rows(to_np(run(p, x, mode)), a_ref, mode)
            assert e <= bound(dt, n, mode), (rows, mode, e)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", [64, 4096])
def test_nonfinite_rows_stay_local(pd, n, dt):
    import torch
    p = plan(pd, n, dt)
    rows = 9
    xc = normal_rows(4, rows, n, dt)
    bad = xc.clone()
    bad[3, 17] = float("nan")
    bad[6, 0] = float("inf")
    for mode in MODES:
        clean, got = run(p, xc, mode), run(p, bad, mode)
        for r in range(rows):
            if r in (3, 6):
                assert not torch.isfinite(torch.view_as_real(got[r]) if mode == "analytic" else got[r]).all()
            else:
                assert torch.equal(got[r], clean[r]), r


def test_overlap_and_argument_errors(pd):
    import torch
    from pragma_dsp_amd import PdspError, _capi
    from pragma_dsp_amd.batch import BatchedFft
    n = 256
    p = plan(pd, n, "f32")
    buf = torch.zeros((12 * n,), device="cuda")
    x = buf[:4 * n].view(4, n)
    for fn in (p.hilbert_imag, p.envelope, p.instantaneous_phase):
        with pytest.raises(PdspError) as e:
            fn(x, out=buf[n:5 * n].view(4, n))  # shifted by one row: partial overlap
        assert e.value.code == _capi.ERR_BAD_ARG and "output overlaps input" in str(e.value)
        with pytest.raises(PdspError) as e:
            fn(x, out=buf[1:4 * n + 1].view(4, n))
        assert e.value.code == _capi.ERR_BAD_ARG and "output overlaps input" in str(e.value)
        _, xs = strided(4, n, n + 4, "f32")
        with pytest.raises(PdspError) as e:  # same base, other stride
            fn(xs, out=xs.as_strided((4, n), (n, 1)))
        assert e.value.code == _capi.ERR_BAD_ARG
        with pytest.raises(PdspError) as e:
            fn(x.double())
        assert e.value.code == _capi.ERR_BAD_ARG
        with pytest.raises(PdspError) as e:
            fn(torch.zeros((4, 2 * n), device="cuda"))  # len > N
        assert e.value.code == _capi.ERR_BAD_ARG and str(e.value) == "len must be 1 ... N = 256, got 512"
        with pytest.raises(PdspError) as e:
            fn(torch.zeros((4, 0), device="cuda"))
        assert e.value.code == _capi.ERR_BAD_ARG
        with pytest.raises(PdspError) as e:
            fn(torch.zeros((n,), device="cuda"))
        assert e.value.code == _capi.ERR_BAD_ARG
        with pytest.raises(PdspError) as e:
            fn(x, out=torch.zeros((3, n), device="cuda"))
        assert e.value.code == _capi.ERR_BAD_ARG
        with pytest.raises(PdspError) as e:
            fn(x[:, :100], out=torch.zeros((4, 100), device="cuda"))  # the output has N samples whatever len is
        assert e.value.code == _capi.ERR_BAD_ARG
        with pytest.raises(PdspError) as e:
            fn(torch.zeros((4, 2 * n), device="cuda")[:, ::2])
        assert e.value.code == _capi.ERR_BAD_ARG
        with pytest.raises(PdspError) as e:
            fn(torch.zeros((0, n), device="cuda"))
        assert e.value.code == _capi.ERR_BAD_ARG
    # analytic: a complex output, never in place
    with pytest.raises(PdspError) as e:
        p.hilbert(x, out=torch.zeros((4, n), device="cuda"))
    assert e.value.code == _capi.ERR_BAD_ARG
    with pytest.raises(PdspError) as e:
        p.hilbert(x, out=torch.view_as_complex(buf[:8 * n].view(4, n, 2)))  # y begins where x does
    assert e.value.code == _capi.ERR_BAD_ARG and "output overlaps input" in str(e.value)
    with pytest.raises(PdspError) as e:
        p.hilbert(x, out=torch.view_as_complex(buf[2 * n:10 * n].view(4, n, 2)))
    assert e.value.code == _capi.ERR_BAD_ARG and "output overlaps input" in str(e.value)
    for bad_n in (32, 32768):
        q = BatchedFft(bad_n)
        for fn in (q.hilbert, q.hilbert_imag, q.envelope, q.instantaneous_phase):
            with pytest.raises(PdspError) as e:
                fn(torch.zeros((2, bad_n), device="cuda"))
            assert e.value.code == _capi.ERR_UNSUPPORTED_SIZE
            assert str(e.value) == f"the Hilbert transform needs a plan of 64 <= N <= 16384, got {bad_n}"
    # the C ABI directly, with device pointers
    lib = pd.lib
    vp = C.c_void_p
    xp, yp = vp(x.data_ptr()), vp(buf[4 * n:].data_ptr())
    f = lib.pdsp_hilbert_f32
    IMAG, ANALYTIC = 1, 0
    assert f(p._h, 0, xp, n, n, IMAG, yp, n, None) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"batch must be >= 1, got 0"
    for ln in (0, n + 1):
        assert f(p._h, 2, xp, n + 1, ln, IMAG, yp, n, None) == _capi.ERR_BAD_ARG
        assert lib.pdsp_last_error() == b"len must be 1 ... N = 256, got %d" % ln
    for mode in (-1, 4):
        assert f(p._h, 2, xp, n, n, mode, yp, n, None) == _capi.ERR_BAD_ARG
        assert lib.pdsp_last_error() == (b"Hilbert output must be 0 (analytic), 1 (imag), 2 (envelope) or 3 (phase), "
                                         b"got %d" % mode)
    assert f(p._h, 2, xp, n - 1, n, IMAG, yp, n, None) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == (b"strides must be >= len = 256 (x) and >= 256 (y), got x_stride 255, "
                                     b"y_stride 256")
    assert f(p._h, 2, xp, n, n, IMAG, yp, n - 1, None) == _capi.ERR_BAD_ARG
    assert f(p._h, 2, xp, n, n, ANALYTIC, yp, 2 * n - 1, None) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == (b"strides must be >= len = 256 (x) and >= 512 (y), got x_stride 256, "
                                     b"y_stride 511")
    assert f(p._h, 2, xp, 100, 100, IMAG, yp, n, None) == _capi.OK  # x_stride >= len is enough
    assert f(p._h, 2, None, n, n, IMAG, yp, n, None) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"null buffer"
    assert f(p._h, 2, xp, n, n, IMAG, None, n, None) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"null buffer"
    assert f(p._h, 1 << 31, vp(16), n, n, IMAG, vp(1 << 44), n, None) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"batch too large: 2147483648"
    assert f(p._h, 1 << 40, vp(16), 1 << 30, n, IMAG, vp(1 << 44), n, None) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"batch 1099511627776 x stride overflows"
    assert f(p._h, 2, xp, n, n, ANALYTIC, xp, n, None) == _capi.ERR_BAD_ARG  # in place, but analytic: stride first
    assert f(p._h, 2, xp, 2 * n, n, ANALYTIC, xp, 2 * n, None) == _capi.ERR_BAD_ARG
    assert b"output overlaps input" in lib.pdsp_last_error()
    assert f(p._h, 2, xp, n, n, IMAG, xp, n + 2, None) == _capi.ERR_BAD_ARG  # same base, other stride
    assert b"output overlaps input" in lib.pdsp_last_error()
    torch.cuda.synchronize()

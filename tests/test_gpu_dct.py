"""dct / idct on the device (pdsp_dct_kernel.h): every N = 64 ... 16384 x f32 / f64 x type 2 / 3 x norm x dct / idct
against the f64 numpy restatement of test_dct_cpu (itself pinned to scipy.fft there), computed from the same inputs
rounded to the dtype.  Metric: per row max|y - y_ref| / max|y_ref|, bound TOL[dtype] * log2 N.
Both kernel paths are reached on purpose: FAST (16-byte aligned rows, strides multiples of 16 bytes; _fast() mirrors
dct_fast_path in pdsp_kernels_dct.hip) and the general one (a one-element offset, odd strides).  They differ only in
how rows move, so their results are bitwise equal, and so are in place vs out of place, repeated calls and the host
f64 form vs BatchedFft f64."""
import numpy as np
import pytest

from test_dct_cpu import NORMS, dct_ref, idct_ref

pytestmark = pytest.mark.gpu

NS = [64 << i for i in range(9)]  # 64 ... 16384
TOL = {"f32": 9e-8, "f64": 2.4e-16}  # x log2 N: 3x the worst measured, 2.9e-8 / 8.0e-17
SENTINEL = float("nan")


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


def _fast(x, y):
    """Mirror of dct_fast_path: both row pointers 16-byte aligned, both row strides multiples of 16 bytes."""
    es = x.element_size()
    xs = x.stride(0) if x.shape[0] > 1 else x.shape[1]
    ys = y.stride(0) if y.shape[0] > 1 else y.shape[1]
    return x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0 and (xs * es) % 16 == 0 and (ys * es) % 16 == 0


def rel_rows(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    den = np.abs(want).max(axis=-1)
    return (np.abs(got - want).max(axis=-1) / np.where(den > 0, den, 1.0)).max()


def run(p, x, type, norm, inverse=False, out=None):
    return (p.idct if inverse else p.dct)(x, type=type, norm=norm, out=out)


def strided(rows, n, stride, dt, offset=0, fill=SENTINEL):
    """A [rows, n] view at row stride `stride`, `offset` elements into a buffer filled with `fill`."""
    import torch
    buf = torch.full((offset + rows * stride + 8,), fill, dtype=_t(dt), device="cuda")
    return buf, buf.as_strided((rows, n), (stride, 1), offset)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", NS)
def test_every_type_norm_and_direction_against_numpy(pd, n, dt):
    import torch
    p = plan(pd, n, dt)
    rng = np.random.default_rng(n + (dt == "f64"))
    rows = 5
    x = torch.from_numpy(rng.standard_normal((rows, n))).to(_t(dt)).cuda()
    xh = x.double().cpu().numpy()
    worst = 0.0
    for t in (2, 3):
        for norm in NORMS:
            for inverse in (False, True):
                y = run(p, x, t, norm, inverse)
                assert _fast(x, y)
                want = (idct_ref if inverse else dct_ref)(xh, t, norm)
                e = rel_rows(y.cpu().numpy(), want)
                worst = max(worst, e / (n.bit_length() - 1))
                assert e <= TOL[dt] * (n.bit_length() - 1), (n, dt, t, norm, inverse, e)
    print(f"DCTERR {dt} n={n} worst/log2N={worst:.3e}")


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", [64, 512, 4096, 16384])
def test_round_trips(pd, n, dt):
    import torch
    p = plan(pd, n, dt)
    x = torch.from_numpy(np.random.default_rng(7).standard_normal((3, n))).to(_t(dt)).cuda()
    for t in (2, 3):
        for norm in NORMS:
            back = p.idct(p.dct(x, type=t, norm=norm), type=t, norm=norm)
            e = rel_rows(back.cpu().numpy(), x.cpu().numpy())
            assert e <= 2 * TOL[dt] * (n.bit_length() - 1), (t, norm, e)


@pytest.mark.parametrize("n", [64, 1024, 16384])
def test_parseval_ortho_f64(pd, n):
    import torch
    p = plan(pd, n, "f64")
    x = torch.from_numpy(np.random.default_rng(11).standard_normal((4, n))).cuda()
    y = p.dct(x, type=2, norm="ortho")
    ex, ey = (x * x).sum(dim=1).cpu().numpy(), (y * y).sum(dim=1).cpu().numpy()
    assert np.abs(ey - ex).max() <= 1e-13 * ex.max()


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", [64, 2048, 16384])
def test_known_answers(pd, n, dt):
    import torch
    p = plan(pd, n, dt)
    nn = np.arange(n)
    ks = [1, 5, n // 4, n // 2, n - 1]
    # the angle reduced exactly (integer phase mod 4N) so that the inputs are correct to the last bit
    x = np.stack([np.cos(np.pi * ((k * (2 * nn + 1)) % (4 * n)) / (2 * n)) for k in ks] + [np.full(n, 0.75)])
    y = p.dct(torch.from_numpy(x).to(_t(dt)).cuda(), type=2).double().cpu().numpy()
    eps = TOL[dt] * (n.bit_length() - 1) * n
    for r, k in enumerate(ks):
        assert abs(y[r, k] - n) <= eps, (k, y[r, k])
        assert np.abs(np.delete(y[r], k)).max() <= eps, k
    assert abs(y[-1, 0] - 2 * n * 0.75) <= 2 * eps
    assert np.abs(y[-1, 1:]).max() <= 2 * eps


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", NS)
def test_paths_in_place_and_repeats_are_bitwise(pd, n, dt):
    import torch
    p = plan(pd, n, dt)
    rows = 3
    xc = torch.from_numpy(np.random.default_rng(n).standard_normal((rows, n))).to(_t(dt)).cuda()
    for t in (2, 3):
        ref = p.dct(xc, type=t, norm="ortho")
        assert _fast(xc, ref)
        assert torch.equal(p.dct(xc, type=t, norm="ortho"), ref)  # repeated call
        # general path: a one-element offset (misaligned rows) ...
        _, xo = strided(rows, n, n, dt, offset=1)
        xo.copy_(xc)
        yo = p.dct(xo, type=t, norm="ortho")
        assert not _fast(xo, yo)
        assert torch.equal(yo, ref)
        # ... odd strides on both sides
        _, xs = strided(rows, n, n + 1, dt)
        xs.copy_(xc)
        _, ys = strided(rows, n, n + 3, dt)
        p.dct(xs, type=t, norm="ortho", out=ys)
        assert not _fast(xs, ys)
        assert torch.equal(ys, ref)
        # FAST with padded strides (multiples of 16 bytes)
        pad = 16 // xc.element_size()
        _, xf = strided(rows, n, n + pad, dt)
        xf.copy_(xc)
        _, yf = strided(rows, n, n + 2 * pad, dt)
        p.dct(xf, type=t, norm="ortho", out=yf)
        assert _fast(xf, yf)
        assert torch.equal(yf, ref)
        # exact in place, on both paths
        xi = xc.clone()
        assert p.dct(xi, type=t, norm="ortho", out=xi).data_ptr() == xi.data_ptr()
        assert torch.equal(xi, ref)
        p.dct(xs, type=t, norm="ortho", out=xs)
        assert torch.equal(xs, ref)


@pytest.mark.parametrize("n", [64, 1024, 16384])
def test_host_form_matches_device_f64_bitwise(pd, n):
    import torch
    p = plan(pd, n, "f64")
    x = np.random.default_rng(5).standard_normal((4, n))
    xd = torch.from_numpy(x).cuda()
    for t in (2, 3):
        for norm in NORMS:
            assert np.array_equal(pd.dct(x, type=t, norm=norm), p.dct(xd, type=t, norm=norm).cpu().numpy())
            assert np.array_equal(pd.idct(x, type=t, norm=norm), p.idct(xd, type=t, norm=norm).cpu().numpy())
    # 1-D input and norm=None (backward), as scipy
    assert np.array_equal(pd.dct(x[1]), p.dct(xd[1:2]).cpu().numpy()[0])
    assert np.array_equal(pd.idct(x[2], type=3, norm=None), p.idct(xd[2:3], type=3).cpu().numpy()[0])


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", [64, 256, 2048, 16384])
def test_guard_bands(pd, n, dt):
    import torch
    p = plan(pd, n, dt)
    rows = 4
    xc = torch.from_numpy(np.random.default_rng(2).standard_normal((rows, n))).to(_t(dt)).cuda()
    for t in (2, 3):
        ref = p.dct(xc, type=t)
        for xpad, ypad, off in ((16 // xc.element_size(), 16 // xc.element_size(), 0), (3, 5, 1)):
            _, xs = strided(rows, n, n + xpad, dt)  # NaN in the stride gaps of x
            xs.copy_(xc)
            ybuf, ys = strided(rows, n, n + ypad, dt, offset=off)  # NaN sentinels around and between y's rows
            before = ybuf.clone()
            p.dct(xs, type=t, out=ys)
            assert torch.equal(ys, ref)
            mask = torch.ones_like(ybuf, dtype=torch.bool)
            for r in range(rows):
                mask[off + r * (n + ypad): off + r * (n + ypad) + n] = False
            ib = torch.int32 if dt == "f32" else torch.int64
            assert torch.equal(ybuf.view(ib)[mask], before.view(ib)[mask])  # bitwise: gaps and bands untouched


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", [64, 4096])
def test_nonfinite_rows_stay_local(pd, n, dt):
    import torch
    p = plan(pd, n, dt)
    rows = 9
    xc = torch.from_numpy(np.random.default_rng(4).standard_normal((rows, n))).to(_t(dt)).cuda()
    bad = xc.clone()
    bad[3, 17] = float("nan")
    bad[6, 0] = float("inf")
    for t in (2, 3):
        clean, got = p.dct(xc, type=t), p.dct(bad, type=t)
        for r in range(rows):
            if r in (3, 6):
                assert not torch.isfinite(got[r]).all()
            else:
                assert torch.equal(got[r], clean[r]), r


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", NS)
def test_batches_with_dead_rows(pd, n, dt):
    import torch
    p = plan(pd, n, dt)
    R = rows_per_wg(n)
    for rows in sorted({1, R - 1, R + 1, 67} - {0}):
        x = torch.from_numpy(np.random.default_rng(rows).standard_normal((rows, n))).to(_t(dt)).cuda()
        xh = x.double().cpu().numpy()
        for t in (2, 3):
            y = p.dct(x, type=t, norm="forward")
            e = rel_rows(y.cpu().numpy(), dct_ref(xh, t, "forward"))
            assert e <= TOL[dt] * (n.bit_length() - 1), (rows, t, e)


def test_overlap_and_argument_errors(pd):
    import torch
    from pragma_dsp_amd import PdspError, _capi
    n = 256
    p = plan(pd, n, "f32")
    buf = torch.zeros((5 * n,), device="cuda")
    x = buf[:4 * n].view(4, n)
    with pytest.raises(PdspError) as e:
        p.dct(x, out=buf[n:].view(4, n))  # shifted by one row: partial overlap
    assert e.value.code == _capi.ERR_BAD_ARG and "output overlaps input" in str(e.value)
    with pytest.raises(PdspError) as e:
        p.dct(x, out=buf[1:4 * n + 1].view(4, n))
    assert e.value.code == _capi.ERR_BAD_ARG and "output overlaps input" in str(e.value)
    _, xs = strided(4, n, n + 4, "f32")
    with pytest.raises(PdspError) as e:  # same base, other stride
        p.dct(xs, out=xs.as_strided((4, n), (n, 1)))
    assert e.value.code == _capi.ERR_BAD_ARG
    with pytest.raises(PdspError) as e:
        p.dct(x, type=1)
    assert e.value.code == _capi.ERR_BAD_ARG and str(e.value) == "DCT type must be 2 or 3, got 1"
    with pytest.raises(PdspError) as e:
        p.idct(x, type=4)
    assert e.value.code == _capi.ERR_BAD_ARG
    with pytest.raises(PdspError) as e:
        p.dct(x, norm="unit")
    assert e.value.code == _capi.ERR_BAD_ARG and "DCT norm must be" in str(e.value)
    with pytest.raises(PdspError) as e:
        p.dct(x.double())
    assert e.value.code == _capi.ERR_BAD_ARG
    with pytest.raises(PdspError) as e:
        p.dct(torch.zeros((4, 128), device="cuda"))
    assert e.value.code == _capi.ERR_INPUT_LENGTH
    with pytest.raises(PdspError) as e:
        p.dct(torch.zeros((n,), device="cuda"))
    assert e.value.code == _capi.ERR_BAD_ARG
    with pytest.raises(PdspError) as e:
        p.dct(x, out=torch.zeros((3, n), device="cuda"))
    assert e.value.code == _capi.ERR_BAD_ARG
    with pytest.raises(PdspError) as e:
        p.dct(torch.zeros((4, 2 * n), device="cuda")[:, ::2])
    assert e.value.code == _capi.ERR_BAD_ARG
    with pytest.raises(PdspError) as e:
        p.dct(torch.zeros((0, n), device="cuda"))
    assert e.value.code == _capi.ERR_BAD_ARG
    from pragma_dsp_amd.batch import BatchedFft
    for bad_n in (32, 32768):
        q = BatchedFft(bad_n)
        with pytest.raises(PdspError) as e:
            q.dct(torch.zeros((2, bad_n), device="cuda"))
        assert e.value.code == _capi.ERR_UNSUPPORTED_SIZE
        assert str(e.value) == f"DCT needs a plan of 64 <= N <= 16384, got {bad_n}"
    # the C ABI directly: strides below N, a grid of 2^31 rows
    lib = pd.lib
    import ctypes as C
    vp = C.c_void_p
    assert lib.pdsp_dct_f32(p._h, 2, vp(x.data_ptr()), n - 1, 2, 0, vp(x.data_ptr()), n - 1, None) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"strides must be >= N = 256, got x_stride 255, y_stride 255"
    assert lib.pdsp_dct_f32(p._h, 1 << 31, vp(16), n, 2, 0, vp(1 << 44), n, None) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"batch too large: 2147483648"
    assert lib.pdsp_dct_f32(p._h, 1 << 40, vp(16), 1 << 30, 2, 0, vp(1 << 44), n, None) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"batch 1099511627776 x stride overflows"

"""FIR filtering on the MI355X (fused overlap-save, include/pdsp_hip.h "FIR filtering") against numpy in f64:
np.convolve for small cases, an f64 rfft product of the full length for large ones.  Error metric:
max|y - ref| / (max|x| * sum|h|) <= 1e-5 in f32 and <= 1e-13 in f64."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-5, torch.float64: 1e-13}


@pytest.fixture(scope="module")
def pd():
    import pragma_dsp_amd
    return pragma_dsp_amd


def ref_full(x, h):
    """f64 full linear convolution of the rows of x with h."""
    n = x.shape[-1] + h.size - 1
    if x.shape[-1] * h.size <= 1 << 22:
        return np.stack([np.convolve(r, h) for r in x.reshape(-1, x.shape[-1])]).reshape(*x.shape[:-1], n)
    L = 1 << (n - 1).bit_length()
    return np.fft.irfft(np.fft.rfft(x, L) * np.fft.rfft(h, L), L)[..., :n]


def err(y, want, x, h):
    return np.abs(np.asarray(y, dtype=np.float64) - want).max() / (np.abs(x).max() * np.abs(h).sum())


def run(pd, x, h, dtype, mode="full", block=None):
    f = pd.FirFilter(h, "cuda:0", dtype, block)
    y = f.apply(torch.from_numpy(x).to(dtype).cuda(), mode)
    torch.cuda.synchronize()
    return y.cpu().numpy(), f


def check_mode(pd, x, h, dtype, mode, block=None):
    from pragma_dsp_amd.filters import output_range
    xq = x.astype(np.float32).astype(np.float64) if dtype == torch.float32 else x
    hq = h.astype(np.float32).astype(np.float64) if dtype == torch.float32 else h
    off, n = output_range(x.shape[-1], h.size, mode)
    want = ref_full(xq, hq)[..., off:off + n]
    y, _ = run(pd, x, h, dtype, mode, block)
    assert y.shape == want.shape
    e = err(y, want, xq, hq)
    assert e <= TOL[dtype], (mode, x.shape, h.size, block, e)


CASES = [(torch.float32, n) for n in (64, 1024, 4096, 16384)] + [(torch.float64, n) for n in (64, 4096, 8192, 16384)]


@pytest.mark.parametrize("dtype,n", CASES)
def test_taps_and_lengths_against_numpy(pd, dtype, n):
    rng = np.random.default_rng(n + (7 if dtype == torch.float64 else 0))
    for p in sorted({1, 2, 7, 10, n // 2 - 1, n // 2}):
        hop = n - (p | 1) + 1
        h = rng.standard_normal(p)
        for length in sorted({1, max(p - 1, 1), hop, 3 * hop + 1}):
            x = rng.standard_normal(length)
            check_mode(pd, x, h, dtype, "full", block=n)
    # the four modes, len < P included
    p = n // 4 + 1
    h = rng.standard_normal(p)
    for length in (p // 2, 5 * n + 3):
        x = rng.standard_normal(length)
        for mode in ("full", "same", "valid", "filter"):
            check_mode(pd, x, h, dtype, mode, block=n)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_long_signal_and_strided_batch(pd, dtype):
    rng = np.random.default_rng(5)
    h = rng.standard_normal(301)
    x = rng.standard_normal((1 << 20) + 17)
    check_mode(pd, x, h, dtype, "same")
    # rows at a stride bigger than len, output rows at a stride bigger than y_len, odd offsets
    rows, length = 6, 9001
    big = torch.from_numpy(rng.standard_normal((rows, length + 13))).to(dtype).cuda()
    xv = big[:, 1:1 + length]
    f = pd.FirFilter(h[:200], "cuda:0", dtype)
    out_big = torch.full((rows, length + 200 + 40), 7.0, dtype=dtype, device="cuda:0")
    out = out_big[:, 3:3 + length + 199]
    f.apply(xv, "full", out=out)
    torch.cuda.synchronize()
    xs = xv.cpu().numpy().astype(np.float64)
    hq = h[:200].astype(np.float32).astype(np.float64) if dtype == torch.float32 else h[:200]
    assert err(out.cpu().numpy(), ref_full(xs, hq), xs, hq) <= TOL[dtype]
    ob = out_big.cpu().numpy()
    assert (ob[:, :3] == 7).all() and (ob[:, 3 + length + 199:] == 7).all()  # nothing outside the rows
    # a contiguous leading shape [2, 3, len]
    x3 = rng.standard_normal((2, 3, 777))
    check_mode(pd, x3, h[:50], dtype, "valid")


def test_identities_and_linearity(pd):
    rng = np.random.default_rng(11)
    x = rng.standard_normal((3, 5000))
    xt = torch.from_numpy(x).cuda()
    y = pd.FirFilter([1.0], "cuda:0", torch.float64).apply(xt, "filter")
    assert np.abs(y.cpu().numpy() - x).max() <= 1e-14
    for dly in (1, 2, 37, 600):
        e = np.zeros(dly + 1)
        e[dly] = 1.0
        y = pd.FirFilter(e, "cuda:0", torch.float64).apply(xt, "full").cpu().numpy()
        assert np.abs(y[:, dly:dly + 5000] - x).max() <= 1e-14 and np.abs(y[:, :dly]).max() <= 1e-14
    h = rng.standard_normal(129)
    f = pd.FirFilter(h, "cuda:0", torch.float32)
    a = torch.from_numpy(rng.standard_normal(20000)).float().cuda()
    b = torch.from_numpy(rng.standard_normal(20000)).float().cuda()
    lhs = f.apply(2.0 * a - 3.0 * b)
    rhs = 2.0 * f.apply(a) - 3.0 * f.apply(b)
    scale = 5.0 * max(a.abs().max().item(), b.abs().max().item()) * np.abs(h).sum()
    assert (lhs - rhs).abs().max().item() / scale <= 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_frequency_response(pd, dtype):
    rng = np.random.default_rng(3)
    for n, p in ((64, 32), (4096, 100), (16384, 8192)):
        h = rng.standard_normal(p)
        f = pd.FirFilter(h, "cuda:0", dtype, block=n)
        hre, him = f.frequency_response()
        got = hre.cpu().numpy().astype(np.float64) + 1j * him.cpu().numpy().astype(np.float64)
        hq = h.astype(np.float32).astype(np.float64) if dtype == torch.float32 else h
        want = np.fft.rfft(hq, n)
        assert got.shape == (n // 2 + 1,)
        assert np.abs(got - want).max() / np.abs(hq).sum() <= (1e-6 if dtype == torch.float32 else 1e-14)


def test_block_size_independence(pd):
    rng = np.random.default_rng(8)
    h = rng.standard_normal(300)
    x = rng.standard_normal((2, 50000))
    xt = torch.from_numpy(x).float().cuda()
    ys = [pd.FirFilter(h, "cuda:0", torch.float32, block=n).apply(xt, "same").cpu().numpy().astype(np.float64)
          for n in (1024, 2048, 4096, 8192, 16384)]
    scale = np.abs(x).max() * np.abs(h).sum()
    for y in ys[1:]:
        assert np.abs(y - ys[0]).max() / scale <= 1e-5
    assert pd.FirFilter(h, "cuda:0").size == 4096  # the default rule: smallest power of two >= 8 P, >= 4096


def test_host_form_and_one_shot(pd):
    rng = np.random.default_rng(21)
    for length, p in ((1, 1), (5, 9), (1000, 64), (70001, 2048), (3000, 8192)):
        x, h = rng.standard_normal(length), rng.standard_normal(p)
        full = ref_full(x[None], h)[0]
        for mode in ("full", "same", "valid", "filter"):
            y = pd.firFilter(x, h, mode)
            from pragma_dsp_amd.filters import output_range
            off, n = output_range(length, p, mode)
            assert y.shape == (n,) and err(y, full[off:off + n], x, h) <= 1e-13, (length, p, mode)
    xb = rng.standard_normal((4, 333))
    yb = pd.firFilter(xb, [0.5, -1.0, 0.25], "filter")
    assert err(yb, ref_full(xb, np.array([0.5, -1.0, 0.25]))[:, :333], xb, np.array([1.75])) <= 1e-13
    y1 = pd.fir_filter(torch.from_numpy(xb).cuda(), [0.5, -1.0, 0.25], "valid")
    assert err(y1.cpu().numpy(), ref_full(xb, np.array([0.5, -1.0, 0.25]))[:, 2:333], xb, np.array([1.75])) <= 1e-13


def test_device_errors(pd):
    from pragma_dsp_amd import _capi
    with pytest.raises(pd.PdspError) as e:
        pd.FirFilter(np.ones(40), "cuda:0", torch.float32, block=64)
    assert e.value.code == _capi.ERR_UNSUPPORTED_SIZE
    f = pd.FirFilter(np.ones(3), "cuda:0", torch.float32, block=64)
    with pytest.raises(pd.PdspError, match="unknown FIR mode"):
        f.apply(torch.ones(10, device="cuda:0"), "circular")
    # a strided extent beyond LLONG_MAX / 8 elements has no byte size: refused before anything is launched (the extent
    # itself, 2^61 + 10, still computes -- the overlap check used to multiply it by the element size and wrap)
    lib, p = _capi.lib, lambda t: t.data_ptr()
    x, y = torch.ones(20, device="cuda:0"), torch.zeros(20, device="cuda:0")
    for x_stride, y_stride in ((1 << 61, 10), (10, 1 << 61)):
        rc = lib.pdsp_fir_filter_f32(f.plan._h, 2, p(x), 10, x_stride, p(f.h_re), p(f.h_im), 3, 0, 10, p(y), y_stride, None)
        assert rc == _capi.ERR_BAD_ARG and lib.pdsp_last_error().decode() == "batch 2 x stride overflows"
    torch.cuda.synchronize()
    assert float(y.abs().max()) == 0.0

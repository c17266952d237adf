"""Polyphase rate change on the GPU (pdsp_upfirdn_kernel.h) against the f64 restatement of the definition in
tests/test_resample_cpu.py.  Inputs are built in f64 and rounded to the dtype first, the taps are rounded as the
handle rounds them, and the reference is computed in f64 from those rounded values, so the bound holds the kernel's
arithmetic alone: for every output m

    |y[m] - ref[m]| <= (T + 2) * eps * A[m],   T = ceil(ntaps / up),  A[m] = sum |h| |x| over the output's terms,

eps = 2^-23 (f32) or 2^-52 (f64).  Derived, not measured: T fma terms in any fixed order err by at most T u A[m],
u = eps / 2; the f64 reference errs by as much again at its own u; two more cover the rounding of the result and the
multiplication by up.  No sample is excluded, and where A[m] == 0 the output must be exactly 0.
The worst measured ratio to the bound, per case, is recorded in DESIGN.md 4.9."""
import numpy as np
import pytest
import torch

import pragma_dsp_amd as pd
from pragma_dsp_amd import _capi
from pragma_dsp_amd import resample as R
from test_resample_cpu import resample_ref, user_taps

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
EPS = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52}
NP = {torch.float32: np.float32, torch.float64: np.float64}


def signal(shape, dt, seed):
    x = np.random.default_rng(seed).standard_normal(shape)
    return x.astype(NP[dt]).astype(np.float64)


def dev(x, dt):
    return torch.from_numpy(x).to(dt).cuda()


def check(r, x, dt, what):
    """Runs r on x ([rows, len], f64 values exact in dt) and holds every output to the bound; returns the outputs."""
    y = r.apply(dev(x, dt))
    torch.cuda.synchronize()
    n = x.shape[-1]
    assert tuple(y.shape) == (x.shape[0], r.output_len(n)) and y.dtype == dt
    h = r.taps.astype(NP[dt]).astype(np.float64)
    ref = resample_ref(x, r.up, r.down, h, r.t0, y.shape[1])
    a = resample_ref(x, r.up, r.down, h, r.t0, y.shape[1], abs=True)
    got = y.cpu().numpy().astype(np.float64)
    t = -(-r.ntaps // r.up)
    bound = (t + 2) * EPS[dt] * a
    err = np.abs(got - ref)
    worst = float((err[a > 0] / bound[a > 0]).max()) if (a > 0).any() else 0.0
    print(f"{what} {dt} len {n}: worst |err| / bound = {worst:.3f}")
    assert np.all(got[a == 0] == 0.0)
    assert np.all(err <= bound), (what, n, worst)
    return y


RATIOS = [(2, 1), (1, 2), (3, 2), (2, 3), (7, 1), (1, 8), (160, 147), (147, 160)]


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("up,down", RATIOS)
def test_default_taps(up, down, dt):
    r = pd.Resampler(up, down, device="cuda:0", dtype=dt)
    assert (r.up, r.down, r.ntaps) == (up, down, 20 * max(up, down) + 1)
    for n in (1, 2, 63, 64, 65, 2000 if max(up, down) > 100 else 1000):
        check(r, signal((3, n), dt, n + up), dt, f"{up}/{down}")


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("up,down", [(3, 2), (1, 2), (2, 1)])
def test_many_tiles(up, down, dt):
    r = pd.Resampler(up, down, device="cuda:0", dtype=dt)
    check(r, signal((2, 70001), dt, 5), dt, f"{up}/{down} tiles")


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n", [5000, 20000])
def test_one_output_spans_8001_samples(n, dt):
    r = pd.Resampler(1, 400, device="cuda:0", dtype=dt)
    assert r.ntaps == 8001
    check(r, signal((3, n), dt, n), dt, "1/400")


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("ntaps,up", [(1, 1), (16, 1), (17, 1), (8192, 1), (3, 7)])
def test_user_taps(ntaps, up, dt):
    h = np.array([0.5]) if ntaps == 1 else user_taps(ntaps)
    if up == 1:
        r = pd.Upfirdn(h, 1, 1, device="cuda:0", dtype=dt)  # Resampler(1, 1) is the identity whatever the taps
        assert r.ntaps == ntaps
    else:
        r = pd.Resampler(up, 1, taps=h, device="cuda:0", dtype=dt)  # phases 3 ... 6 have no tap at all
        assert np.array_equal(r.taps, h * up)
    check(r, signal((3, 300), dt, ntaps), dt, f"taps {ntaps} up {up}")


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("up,down,n", [(3, 2, 300), (1, 1, 300), (5, 1, 1), (8191, 8192, 3), (4096, 8192, 9)])
def test_upfirdn_full_output(up, down, n, dt):
    # the last two, 8192 taps: 8191/8192 reads its taps from global memory in f64 (no room for a span beside them) and
    # runs plain R = 1 in f32; 4096/8192 runs R = 1 with the taps in LDS in both, in f64 at the unpadded stride
    # tp == tn (tests/test_gpu_resample_paths.py asks the library which)
    h = user_taps(8192 if up > 100 else 17)
    r = pd.Upfirdn(h, up, down, device="cuda:0", dtype=dt)
    y = check(r, signal((3, n), dt, up), dt, f"upfirdn {up}/{down}")
    assert y.shape[1] == ((n - 1) * up + h.size - 1) // down + 1


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_equal_ratio_is_the_identity(dt):
    r = pd.Resampler(6, 6, taps=user_taps(17), device="cuda:0", dtype=dt)
    assert (r.up, r.down, r.ntaps) == (1, 1, 1)
    x = dev(signal((3, 1000), dt, 6), dt)
    assert torch.equal(r(x), x)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("up,down", [(3, 2), (2, 1), (1, 8), (160, 147)])
def test_bitwise_properties(up, down, dt):
    r = pd.Resampler(up, down, device="cuda:0", dtype=dt)
    n = 9001
    x = dev(signal((3, n), dt, 77), dt)
    y = r.apply(x)
    assert torch.equal(r.apply(x), y)                                       # repeated calls
    for row in range(3):
        assert torch.equal(r.apply(x[row:row + 1].clone()), y[row:row + 1])  # a row alone
        assert torch.equal(r.apply(x[row].clone()), y[row])                  # 1-D
    buf = torch.zeros(3 * (n + 13) + 1, dtype=dt, device="cuda")
    view = buf[1:].view(3, n + 13)[:, :n]                                    # padded stride, one element off
    view.copy_(x)
    assert not view.is_contiguous() and torch.equal(r.apply(view), y)
    if dt == torch.float64:
        host = pd.resamplePoly(x.cpu().numpy(), up, down)
        assert np.array_equal(host, y.cpu().numpy())
        assert np.array_equal(pd.resamplePoly(x[0].cpu().numpy(), up, down), y[0].cpu().numpy())
    assert torch.equal(pd.resample_poly(x, up, down), y)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("down", [2, 3, 8])
def test_decimation_is_every_down_th_output_of_the_filter(down, dt):
    h = user_taps(161)
    x = dev(signal((3, 5000), dt, down), dt)
    every = pd.Upfirdn(h, 1, 1, device="cuda:0", dtype=dt).apply(x)
    kept = pd.Upfirdn(h, 1, down, device="cuda:0", dtype=dt).apply(x)
    assert torch.equal(kept, every[:, ::down])   # same terms in the same order
    assert torch.equal(pd.upfirdn(h, x, 1, down), kept)
    if dt == torch.float64:
        assert np.array_equal(pd.upfirdnHost(h, x.cpu().numpy(), 1, down), kept.cpu().numpy())


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("up,down", [(3, 2), (2, 1), (1, 8)])
def test_no_stray_writes(up, down, dt):
    r = pd.Resampler(up, down, device="cuda:0", dtype=dt)
    n = 4099
    x = dev(signal((3, n), dt, 3), dt)
    want = r.apply(x)
    m = r.output_len(n)
    buf = torch.full((4, m + 9), float("nan"), dtype=dt, device="cuda")  # padded rows and a guard row
    out = buf[:3, :m]
    assert r.apply(x, out=out) is out
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert torch.isnan(buf[:3, m:]).all() and torch.isnan(buf[3]).all()


def test_a_bad_out_is_refused():
    r = pd.Resampler(3, 2, device="cuda:0")
    x = torch.ones(2, 100, device="cuda")
    m = r.output_len(100)
    for out in (torch.empty(2, m + 1, device="cuda"), torch.empty(3, m, device="cuda"),
                torch.empty(2, m, device="cuda", dtype=torch.float64), torch.empty(2, m)):
        with pytest.raises(pd.PdspError) as e:
            r.apply(x, out=out)
        assert e.value.code == _capi.ERR_BAD_ARG
    buf = torch.ones(2 * 200, device="cuda")
    with pytest.raises(pd.PdspError) as e:   # out shares bytes with x
        r.apply(buf[:200].view(2, 100), out=buf[100:100 + 2 * m].view(2, m))
    assert e.value.code == _capi.ERR_BAD_ARG and "overlaps" in str(e.value)
    for bad in (torch.ones(2, 100), torch.ones(2, 100, device="cuda", dtype=torch.float64)):
        with pytest.raises(pd.PdspError):
            r.apply(bad)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_a_call_is_ordered_on_the_current_stream(dt):
    r = pd.Resampler(3, 2, device="cuda:0", dtype=dt)
    new = dev(signal((3, 20000), dt, 11), dt)
    want = r.apply(new)
    x = torch.zeros_like(new)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        torch.cuda._sleep(50_000_000)  # tens of milliseconds: a call on another stream would read the zeros
        x.copy_(new, non_blocking=True)
        y = r.apply(x)
    side.synchronize()
    assert torch.equal(y, want)

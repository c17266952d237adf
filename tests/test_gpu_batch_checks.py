"""batch.py's element-wise helpers on the device: f64 operands reach the f64 entry points (hypot, atan2, x * w)
and every malformed operand -- wrong dtype, another device, too few elements, a non-contiguous view, a bad
spectrum(out=) -- is refused before any library call.  The library is replaced by a recorder for the refusals
(after the plans they need exist), so a missing check is a recorded call, never a launch on a bad pointer."""
import numpy as np
import pytest

from test_batch_checks_cpu import Recorder

pytestmark = pytest.mark.gpu


def _ulps(got, want):
    return float((np.abs(got - want) / np.spacing(np.abs(want))).max())


def test_f64_helpers_match_numpy():
    import torch
    from pragma_dsp_amd import batch as B
    rng = np.random.default_rng(11)
    re = rng.standard_normal((3, 1001))
    im = rng.standard_normal((3, 1001))
    # the ends of the double range: squares that overflow / underflow, and exact zeros
    re[0, :6] = [1e300, 1e-300, 0.0, -0.0, 3.0, -1e308]
    im[0, :6] = [1e300, 1e-300, 0.0, 5.0, 4.0, 1e308]
    w = rng.random(1001)
    dre, dim, dw = (torch.from_numpy(v).cuda() for v in (re, im, w))
    mag = B.magnitude(dre, dim).cpu().numpy()
    assert mag.dtype == np.float64
    assert np.isfinite(mag).all() and mag[0, 0] > 1e300 and mag[0, 1] > 0
    assert _ulps(mag, np.hypot(re, im)) <= 2
    ph = B.phase(dre, dim).cpu().numpy()
    assert _ulps(ph, np.arctan2(im, re)) <= 3 and ph[0, 2] == 0
    out = torch.empty_like(dre)
    got = B.apply_window(dre, dw, out=out)
    assert got is out and np.array_equal(out.cpu().numpy(), re * w)  # one correctly rounded product


def test_f64_chain_projections():
    import torch
    from pragma_dsp_amd.fluent import DeviceChain
    from pragma_dsp_amd import PdspError
    rng = np.random.default_rng(12)
    re, im = rng.standard_normal((2, 64)), rng.standard_normal((2, 64))
    c = DeviceChain(torch.from_numpy(re).cuda(), torch.from_numpy(im).cuda())
    assert _ulps(c.mag().cpu().numpy(), np.hypot(re, im)) <= 2
    assert _ulps(c.arg().cpu().numpy(), np.arctan2(im, re)) <= 3
    with pytest.raises(PdspError):  # no f64 complex-op kernel: refused, not reinterpreted as floats
        c.mul(c.clone())


def _bad_calls(torch, B, plan):
    f32 = torch.ones((4, 64), device="cuda")
    f64 = torch.ones((4, 64), device="cuda", dtype=torch.float64)
    short = torch.ones((4, 63), device="cuda")
    tview = torch.ones((64, 4), device="cuda").t()  # [4, 64], not contiguous
    w = torch.ones(64, device="cuda")
    frames = torch.ones((3, 64), device="cuda")
    return [
        ("magnitude dtype", lambda: B.magnitude(f32, f64)),
        ("magnitude short im", lambda: B.magnitude(f32, short)),
        ("magnitude short out", lambda: B.magnitude(f32, f32, out=short)),
        ("magnitude out dtype", lambda: B.magnitude(f32, f32, out=f64)),
        ("magnitude transposed", lambda: B.magnitude(tview, f32)),
        ("phase transposed im", lambda: B.phase(f32, tview)),
        ("phase f16", lambda: B.phase(f32.half(), f32.half())),
        ("apply_window dtype", lambda: B.apply_window(f32, w.double())),
        ("apply_window length", lambda: B.apply_window(f32, w[:63])),
        ("apply_window 2-D window", lambda: B.apply_window(f32, f32)),
        ("apply_window transposed", lambda: B.apply_window(tview, w)),
        ("apply_window short out", lambda: B.apply_window(f32, w, out=short)),
        ("complex f64", lambda: B.complex_mul((f64, f64), (f64, f64))),
        ("complex im dtype", lambda: B.complex_add((f32, f64), (f32, f32))),
        ("complex short im", lambda: B.complex_conj((f32, short))),
        ("complex short b.imag", lambda: B.complex_mul((f32, f32), (w, w[:32]))),
        ("complex b not dividing", lambda: B.complex_mul((f32, f32), (w[:48], w[:48]))),
        ("complex transposed b", lambda: B.complex_sub((f32, f32), (tview, f32))),
        ("complex short out", lambda: B.complex_scale((f32, f32), 2.0, out=(f32, short))),
        ("complex transposed out", lambda: B.complex_mul_scalar((f32, f32), 1.0, 2.0, out=(tview, f32))),
        ("spectrum out dtype", lambda: plan.spectrum(frames, out=torch.empty((3, 33), device="cuda", dtype=torch.float64))),
        ("spectrum out short", lambda: plan.spectrum(frames, out=torch.empty((3, 32), device="cuda"))),
        ("spectrum out rows", lambda: plan.spectrum(frames, out=torch.empty((2, 33), device="cuda"))),
        ("spectrum out two-sided", lambda: plan.spectrum(frames, sides="two", out=torch.empty((3, 33), device="cuda"))),
        ("spectrum out transposed", lambda: plan.spectrum(frames, out=torch.empty((33, 3), device="cuda").t())),
        ("spectrum out host", lambda: plan.spectrum(frames, out=torch.empty((3, 33)))),
    ]


def test_bad_operands_never_reach_the_library(pdsp, monkeypatch):
    import torch
    from pragma_dsp_amd import batch as B
    plan = B.BatchedFft(64, "cuda:0")
    calls = _bad_calls(torch, B, plan)
    rec = Recorder()
    monkeypatch.setattr(B, "lib", rec)
    for name, call in calls:
        with pytest.raises(pdsp.PdspError):
            call()
        assert rec.calls == [], name
    monkeypatch.undo()
    plan.close()


def test_other_device_operands_never_reach_the_library(pdsp, monkeypatch):
    import torch
    from pragma_dsp_amd import batch as B
    if torch.cuda.device_count() < 2:
        pytest.skip("needs a second visible device")
    plan = B.BatchedFft(64, "cuda:0")
    a = torch.ones((4, 64), device="cuda:0")
    b = torch.ones((4, 64), device="cuda:1")
    frames = torch.ones((3, 64), device="cuda:0")
    calls = [
        ("magnitude", lambda: B.magnitude(a, b)),
        ("magnitude out", lambda: B.magnitude(a, a, out=b)),
        ("apply_window", lambda: B.apply_window(a, b[0])),
        ("complex b", lambda: B.complex_mul((a, a), (b, b))),
        ("complex out", lambda: B.complex_conj((a, a), out=(a, b))),
        ("spectrum frames", lambda: plan.spectrum(b[:3])),
        ("spectrum out", lambda: plan.spectrum(frames, out=torch.empty((3, 33), device="cuda:1"))),
    ]
    rec = Recorder()
    monkeypatch.setattr(B, "lib", rec)
    for name, call in calls:
        with pytest.raises(pdsp.PdspError):
            call()
        assert rec.calls == [], name
    monkeypatch.undo()
    plan.close()

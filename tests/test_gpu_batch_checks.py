"""The Python device layer hands raw pointers to the library: f64 operands of batch.py's element-wise helpers reach
the f64 entry points (hypot, atan2, x * w), and every malformed operand of every device entry point -- wrong dtype,
another device, too few elements or rows, a non-contiguous view, a foreign plan's window, a bad out -- is refused before
any library call.  The library is replaced by a recorder for the refusals (after the handles they need exist), so a
missing check is a recorded call, never a launch on a bad pointer; the same recorder, keeping the arguments, shows
that every valid call reaches the function and the arguments include/pdsp_hip.h declares."""
import ctypes as C

import numpy as np
import pytest

from test_batch_checks_cpu import Recorder

pytestmark = pytest.mark.gpu

MODULES = ("batch", "filters", "resample", "wavelet", "dft", "czt")  # each looks its entry points up through its own `lib`
QUERIES = ("pdsp_fir_output_range", "pdsp_resample_output_len")      # host arithmetic on integers: no pointer, no launch


class ArgRecorder(Recorder):
    """The recorder, keeping (name, arguments); the two length queries go through to the library."""

    def __init__(self, real):
        super().__init__()
        self._real = real

    def __getattr__(self, name):
        if name in QUERIES:
            return getattr(self._real, name)

        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def _patch_all(monkeypatch):
    import importlib
    from pragma_dsp_amd import _capi
    rec = ArgRecorder(_capi.lib)
    for m in MODULES:
        monkeypatch.setattr(importlib.import_module("pragma_dsp_amd." + m), "lib", rec)
    return rec


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


def _bad_calls(torch, B, plan, other):
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
    ] + _bad_plan_calls(torch, plan, other, frames, f32)


def _bad_plan_calls(torch, plan, other, frames, re):
    """forward / inverse planes with fewer rows than the input, windows of the spectrum family that are not N values of
    the plan's dtype in a row (or belong to another plan), and stft's hop and signal."""
    short = torch.ones((2, 64), device="cuda")
    w = torch.ones(64, device="cuda")
    sig = torch.ones(256, device="cuda")
    foreign = other.window("hann")  # resolved here: under the recorder it would be a library call
    bad = []
    for name in ("forward", "inverse"):
        fn = getattr(plan, name)
        bad += [(name + " short im", lambda fn=fn: fn(re, short)),
                (name + " short out.real", lambda fn=fn: fn(re, re, out=(short, torch.empty_like(re)))),
                (name + " short out.imag", lambda fn=fn: fn(re, re, out=(torch.empty_like(re), short)))]
    for name in ("spectrum", "spectrum_peaks"):
        fn = getattr(plan, name)
        bad += [(name + " window of 63", lambda fn=fn: fn(frames, w[:63])),
                (name + " window f64", lambda fn=fn: fn(frames, w.double())),
                (name + " window transposed", lambda fn=fn: fn(frames, torch.ones((64, 2), device="cuda").t())),
                (name + " window strided", lambda fn=fn: fn(frames, torch.ones(128, device="cuda")[::2])),
                (name + " window [2, 64]", lambda fn=fn: fn(frames, torch.ones((2, 64), device="cuda"))),
                (name + " window of another plan", lambda fn=fn: fn(frames, foreign))]
    return bad + [("stft hop 0", lambda: plan.stft(sig, 0)),
                  ("stft 2-D signal", lambda: plan.stft(sig.view(4, 64), 16))]


def test_bad_operands_never_reach_the_library(pdsp, monkeypatch):
    import torch
    from pragma_dsp_amd import batch as B
    plan = B.BatchedFft(64, "cuda:0")
    other = B.BatchedFft(64, "cuda:0", torch.float64)
    calls = _bad_calls(torch, B, plan, other)
    rec = Recorder()
    monkeypatch.setattr(B, "lib", rec)
    for name, call in calls:
        with pytest.raises(pdsp.PdspError):
            call()
        assert rec.calls == [], name
    monkeypatch.undo()
    plan.close()
    other.close()


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
        ("spectrum_peaks window", lambda: plan.spectrum_peaks(frames, b[0])),
        ("forward out", lambda: plan.forward(a, a, out=(b, b))),
        ("spectrum window of a plan on cuda:1", lambda w=B.BatchedFft(64, "cuda:1").window("hann"): plan.spectrum(frames, w)),
    ]
    rec = Recorder()
    monkeypatch.setattr(B, "lib", rec)
    for name, call in calls:
        with pytest.raises(pdsp.PdspError):
            call()
        assert rec.calls == [], name
    monkeypatch.undo()
    plan.close()


def test_bad_rows_never_reach_the_library(pdsp, monkeypatch):
    """The handles behind the shared rows launch: an out one row short, an out of the other dtype and a 3-D
    non-contiguous input are refused by FirFilter, Resampler, Dwt and Dft alike, before any library call."""
    import torch
    pd = pdsp

    def planes(rows, n, dtype=torch.float32):
        return torch.empty((rows, n), device="cuda", dtype=dtype)

    def pair(rows, n, dtype=torch.float32):
        return planes(rows, n, dtype), planes(rows, n, dtype)

    # (name, entry point, samples per row, outputs per row, how an out argument is made)
    handles = [("FirFilter", pd.FirFilter(np.ones(9), "cuda:0").apply, 256, 264, planes),
               ("Resampler", pd.Resampler(3, 2, device="cuda:0").apply, 256, 384, planes),
               ("Dwt", pd.Dwt("db2", 2, "cuda:0").forward, 256, 256, planes),
               ("Dft", pd.Dft(12, "cuda:0").forward, 12, 12, pair)]
    calls = []
    for name, fn, n, m, mk in handles:
        x = torch.ones((2, n), device="cuda")
        cube = torch.ones((2, 2, 2 * n), device="cuda")[:, :, ::2]  # [2, 2, n]: rows at a stride, but not 2-D
        calls += [(name + " out one row short", lambda fn=fn, x=x, o=mk(1, m): fn(x, out=o)),
                  (name + " out dtype", lambda fn=fn, x=x, o=mk(2, m, torch.float64): fn(x, out=o)),
                  (name + " 3-D non-contiguous input", lambda fn=fn, cube=cube: fn(cube))]
    rec = _patch_all(monkeypatch)
    for name, call in calls:
        with pytest.raises(pd.PdspError):
            call()
        assert rec.calls == [], name
    monkeypatch.undo()


def _valid_calls(torch, pd):
    """(name, call, expected) for every public device method: contiguous and, where the method takes one, a 2-D view
    with a row stride; out=None and out= given.  expected(result) is the library function and its arguments after the
    handle and before the stream, written out from the declarations in include/pdsp_hip.h: integers and floats as
    they are, pointers as the tensor they must equal (None: null)."""
    from pragma_dsp_amd import batch as B
    f32, f64 = torch.float32, torch.float64

    def t(*shape, dtype=f32):
        return torch.ones(shape, device="cuda", dtype=dtype)

    def view(rows, n, stride, dtype=f32):  # [rows, n] at a row stride
        return t(rows, stride, dtype=dtype)[:, :n]

    p, q = B.BatchedFft(64, "cuda:0"), B.BatchedFft(64, "cuda:0", f64)
    hann = p.window("hann")  # cached by the plan: under the recorder it would be a library call
    re, im, o1, o2 = t(4, 64), t(4, 64), t(4, 64), t(4, 64)
    dre, dim, do1, do2 = (t(4, 64, dtype=f64) for _ in range(4))
    z, zo = t(4, 64, dtype=torch.complex64), t(4, 64, dtype=torch.complex64)
    frames, f40, w = t(3, 64), t(3, 40), t(64)
    amp2 = t(3, 64)
    sig, sre, sim, total = t(256), t(7, 33), t(7, 33), t(256)  # 7 = 1 + (256 - 64) // 32 frames, 256 = 6 * 32 + 64
    x80, y96, x40 = view(4, 64, 80), view(4, 64, 96), view(4, 40, 80)
    row, row2 = t(64), t(64)
    fir = pd.FirFilter(np.ones(9), "cuda:0")
    rs, up = pd.Resampler(3, 2, device="cuda:0"), pd.Upfirdn(np.ones(9), 2, 1, "cuda:0")
    dwt, dft, czt = pd.Dwt("db2", 2, "cuda:0"), pd.Dft(12, "cuda:0"), pd.Czt(12, 5, 0.01, device="cuda:0")
    x, xs, ys = t(2, 256), view(2, 256, 300), view(2, 256, 320)
    r384 = view(2, 384, 400)
    a12, b12 = t(2, 12), t(2, 12)
    d16, e16, g20, h20 = (view(2, 12, 16, f64), view(2, 12, 16, f64), view(2, 12, 20, f64), view(2, 12, 20, f64))
    ph, fh = p._h, fir.plan._h
    return [
        ("forward real", lambda: p.forward(re), lambda r: ("pdsp_fft_forward_real_f32", ph, 4, re, r[0], r[1])),
        ("forward complex out", lambda: p.forward(re, im, out=(o1, o2)),
         lambda r: ("pdsp_fft_forward_complex_f32", ph, 4, re, im, o1, o2)),
        ("forward reshaped views", lambda: p.forward(re.view(2, 2, 64), im, out=(o1.view(1, 4, 64), o2)),
         lambda r: ("pdsp_fft_forward_complex_f32", ph, 4, re, im, o1, o2)),
        ("inverse", lambda: p.inverse(re, im), lambda r: ("pdsp_fft_inverse_f32", ph, 4, re, im, r[0], r[1])),
        ("inverse f64 out", lambda: q.inverse(dre, dim, out=(do1, do2)),
         lambda r: ("pdsp_fft_inverse_f64", q._h, 4, dre, dim, do1, do2)),
        ("forward_interleaved", lambda: p.forward_interleaved(z), lambda r: ("pdsp_fft_forward_interleaved_f32", ph, 4, z, r)),
        ("inverse_interleaved out", lambda: p.inverse_interleaved(z, out=zo),
         lambda r: ("pdsp_fft_inverse_interleaved_f32", ph, 4, z, zo)),
        ("spectrum", lambda: p.spectrum(frames, "hann"),
         lambda r: ("pdsp_spectrum_f32", ph, 3, frames, 64, 64, hann, 0, r[0], None, None)),
        ("spectrum short frames, own window, two-sided, out", lambda: p.spectrum(f40, w, "two", True, True, out=amp2),
         lambda r: ("pdsp_spectrum_f32", ph, 3, f40, 40, 40, w, 1, amp2, r[1], r[2])),
        ("spectrum plan window", lambda: p.spectrum(frames, hann, want_phase=True),
         lambda r: ("pdsp_spectrum_f32", ph, 3, frames, 64, 64, hann, 0, r[0], r[1], None)),
        ("spectrum rect", lambda: p.spectrum(frames),
         lambda r: ("pdsp_spectrum_f32", ph, 3, frames, 64, 64, None, 0, r[0], None, None)),
        ("spectrum_peaks", lambda: p.spectrum_peaks(frames, "hann", sample_rate=48000.0),
         lambda r: ("pdsp_spectrum_peaks_f32", ph, 3, frames, 64, 64, hann, 0, 48000.0, None, None, r[0])),
        ("spectrum_peaks own window, amplitudes", lambda: p.spectrum_peaks(frames, w, "two", want_amp=True),
         lambda r: ("pdsp_spectrum_peaks_f32", ph, 3, frames, 64, 64, w, 1, 1.0, r[4], None, r[0])),
        ("stft", lambda: p.stft(sig, 32, "hann", want_peak=True),
         lambda r: ("pdsp_spectrum_f32", ph, 7, sig, 64, 32, hann, 0, r[0], None, r[2])),
        ("stft_complex", lambda: p.stft_complex(sig, 32),
         lambda r: ("pdsp_stft_complex_f32", ph, 7, sig, 64, 32, hann, r[0], r[1])),
        ("istft", lambda: p.istft(sre, sim, 32), lambda r: ("pdsp_istft_f32", ph, 7, sre, sim, 32, hann, r)),
        ("istft own window, out", lambda: p.istft(sre, sim, 32, w, out=total),
         lambda r: ("pdsp_istft_f32", ph, 7, sre, sim, 32, w, total)),
        ("dct", lambda: p.dct(re), lambda r: ("pdsp_dct_f32", ph, 4, re, 64, 2, 0, r, 64)),
        ("idct strided, ortho, out", lambda: p.idct(x80, 2, "ortho", out=y96),
         lambda r: ("pdsp_dct_f32", ph, 4, x80, 80, 3, 1, y96, 96)),
        ("hilbert", lambda: p.hilbert(re), lambda r: ("pdsp_hilbert_f32", ph, 4, re, 64, 64, 0, r, 128)),
        ("hilbert_imag short strided rows", lambda: p.hilbert_imag(x40),
         lambda r: ("pdsp_hilbert_f32", ph, 4, x40, 80, 40, 1, r, 64)),
        ("envelope in place", lambda: p.envelope(o1, out=o1), lambda r: ("pdsp_hilbert_f32", ph, 4, o1, 64, 64, 2, o1, 64)),
        ("instantaneous_phase strided out", lambda: p.instantaneous_phase(re, out=y96),
         lambda r: ("pdsp_hilbert_f32", ph, 4, re, 64, 64, 3, y96, 96)),
        ("apply_window", lambda: B.apply_window(re, w), lambda r: ("pdsp_apply_window_f32", 4, 64, re, w, r)),
        ("magnitude f64", lambda: B.magnitude(dre, dim), lambda r: ("pdsp_magnitude_f64", 256, dre, dim, r)),
        ("phase out", lambda: B.phase(re, im, out=o1), lambda r: ("pdsp_phase_f32", 256, re, im, o1)),
        ("complex_mul by a row", lambda: B.complex_mul((re, im), (row, row2)),
         lambda r: ("pdsp_complex_op_f32", 2, 256, re, im, row, row2, 64, 0.0, 0.0, r[0], r[1])),
        ("complex_scale out", lambda: B.complex_scale((re, im), 2.0, out=(o1, o2)),
         lambda r: ("pdsp_complex_op_f32", 5, 256, re, im, None, None, 0, 2.0, 0.0, o1, o2)),
        # full: all 256 + 9 - 1 outputs from 0; same: 256 from (9 - 1) // 2
        ("FirFilter.apply", lambda: fir.apply(x),
         lambda r: ("pdsp_fir_filter_f32", fh, 2, x, 256, 256, fir.h_re, fir.h_im, 9, 0, 264, r, 264)),
        ("FirFilter.apply strided, same, out", lambda: fir.apply(xs, "same", out=ys),
         lambda r: ("pdsp_fir_filter_f32", fh, 2, xs, 256, 300, fir.h_re, fir.h_im, 9, 4, 256, ys, 320)),
        # ceil(256 * 3 / 2) = 384; (255 * 2 + 9 - 1) // 1 + 1 = 519
        ("Resampler.apply", lambda: rs.apply(x), lambda r: ("pdsp_upfirdn_f32", rs._h, 2, x, 256, 256, r, 384, 384)),
        ("Resampler.apply strided, out", lambda: rs.apply(xs, out=r384),
         lambda r: ("pdsp_upfirdn_f32", rs._h, 2, xs, 256, 300, r384, 384, 400)),
        ("Upfirdn.apply", lambda: up.apply(x), lambda r: ("pdsp_upfirdn_f32", up._h, 2, x, 256, 256, r, 519, 519)),
        ("Dwt.forward", lambda: dwt.forward(x), lambda r: ("pdsp_dwt_forward_f32", dwt._h, 2, x, 256, 256, r, 256)),
        ("Dwt.inverse strided, out", lambda: dwt.inverse(xs, out=ys),
         lambda r: ("pdsp_dwt_inverse_f32", dwt._h, 2, xs, 256, 300, ys, 320)),
        ("Dft.forward real", lambda: dft.forward(a12),
         lambda r: ("pdsp_dft_c2c_f32", dft._h, 2, a12, None, 12, r[0], r[1], 12, 0)),
        ("Dft.inverse f64 strided, out", lambda: dft.inverse(d16, e16, out=(g20, h20)),
         lambda r: ("pdsp_dft_c2c_f64", dft._h, 2, d16, e16, 16, g20, h20, 20, 1)),
        ("Czt.forward", lambda: czt.forward(a12, b12), lambda r: ("pdsp_czt_f32", czt._h, 2, a12, b12, 12, r[0], r[1], 5)),
    ]


def _plain(v):
    """An argument as an integer or a float: pointers (ctypes, tensors, plan windows, None) by address."""
    if v is None:
        return 0
    if isinstance(v, C.c_void_p):
        return v.value or 0
    return v.data_ptr() if hasattr(v, "data_ptr") else v


def test_valid_calls_reach_the_library_as_declared(pdsp, monkeypatch):
    import torch
    calls = _valid_calls(torch, pdsp)
    stream = torch.cuda.current_stream().cuda_stream
    rec = _patch_all(monkeypatch)
    for name, call, expected in calls:
        del rec.calls[:]
        result = call()
        assert len(rec.calls) == 1, (name, rec.calls)
        fn, args = rec.calls[0]
        want = expected(result)
        assert fn == want[0], name
        assert [_plain(a) for a in args] == [_plain(a) for a in want[1:]] + [stream], name
    monkeypatch.undo()

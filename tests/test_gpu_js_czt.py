"""czt / zoomFft of the JS host (pragma-dsp_amd/js `.czt`, through the N-API addon) against the direct sum with exact
phases of test_czt_cpu (grid_direct: dyadic steps and starts) on seeded inputs at the f64 bound of test_gpu_czt: plain /
Float64Array / Float32Array inputs, real and complex, the defaults, the error texts, and the root's key list, which
`.czt` must not join."""
import functools

import numpy as np
import pytest

import js_host
from test_czt_cpu import GRID, grid_direct, row_err
from test_gpu_czt import bound

pytestmark = [pytest.mark.gpu, js_host.needs_node]
run_cases = functools.partial(js_host.run_cases, "czt_cases.js")


def test_js_czt_against_the_direct_sum(tmp_path):
    rng = np.random.default_rng(59)
    cases, want, ins = [], [], []
    for ln, bins in ((3, 8), (1000, 256), (3000, 1024)):
        z = rng.standard_normal(ln) + 1j * rng.standard_normal(ln)
        for typed in (None, "f64", "f32"):
            zin = z.astype(np.complex64).astype(np.complex128) if typed == "f32" else z
            base = {"real": z.real.tolist(), "imag": z.imag.tolist(), "typed": typed, "fn": None}
            # step = 1 / (2 m), a quarter turn in, radius 0.9995 (1 at L = 3000)
            radius = 0.9995 if ln <= 1000 else 1.0
            cases.append(dict(base, op="czt", options={"m": bins, "step": 0.5 / bins, "start": 0.25, "radius": radius}))
            want.append((grid_direct(zin[None], bins, GRID // (2 * bins), GRID // 4, radius)[0], zin, radius))
            # the band [0.25, 0.75) of fs = 2: step = 1 / (4 m), start = 1 / 8; then [0, 0.5) of a real signal
            cases.append(dict(base, op="zoomFft", fn=[0.25, 0.75], options={"m": bins}))
            want.append((grid_direct(zin[None], bins, GRID // (4 * bins), GRID // 8)[0], zin, 1.0))
            cases.append(dict(base, op="zoomFft", imag=None, fn=0.5, options={"m": bins, "fs": 2, "endpoint": False}))
            want.append((grid_direct(zin.real[None], bins, GRID // (4 * bins))[0], zin.real, 1.0))
    # the defaults on a real signal: m = L, step = 1 / m (exact at L = 1024): the DFT
    x = rng.standard_normal(1024)
    cases.append({"op": "czt", "real": x.tolist(), "imag": None, "typed": None, "fn": None, "options": None})
    want.append((np.fft.fft(x), x, 1.0))
    got, keys = run_cases(cases, tmp_path)
    assert keys == ["spectrum", "spectrumBatch", "spectrumStream", "core", "fourier"]
    for c, g, (w, x, radius) in zip(cases, got, want):
        assert isinstance(g, dict) and "real" in g, (c["op"], len(c["real"]), g)
        g = np.asarray(g["real"]) + 1j * np.asarray(g["imag"])
        assert g.shape == w.shape
        assert row_err(g, w, x, radius) <= bound("f64", len(x), len(w)), (c["op"], len(x), len(w), c["typed"])


def test_js_czt_errors(tmp_path):
    one = {"real": [1.0, 2.0, 3.0], "imag": None, "typed": None, "fn": None}
    cases = [
        dict(one, op="czt", options={"m": 8191}),
        dict(one, op="czt", options={"m": 0}),
        dict(one, op="czt", real=[], options=None),
        dict(one, op="czt", options={"radius": 0}),
        dict(one, op="czt", options={"step": "x"}),
        dict(one, op="czt", options={"m": 2.5}),
        dict(one, op="czt", imag=[1.0, 2.0], options=None),
        dict(one, op="zoomFft", fn=[0.1, 0.2, 0.3], options=None),
        dict(one, op="zoomFft", fn=0.5, options={"fs": 0}),
        dict(one, op="zoomFft", fn=0.5, options={"m": 8191}),
    ]
    got, _ = run_cases(cases, tmp_path)
    assert [g["error"] for g in got] == [
        "CZT length + bins - 1 must be <= 8192, got 3 + 8191 - 1",
        "CZT bins must be >= 1, got 0",
        "CZT length must be >= 1, got 0",
        "CZT radius must be finite and > 0, got 0",
        "step must be a number",
        "m must be an integer",
        "real and imag must have the same length, got 3 and 2",
        "fn must be a number or a pair [f1, f2]",
        "fs must be finite and non-zero (and m > 1 with endpoint)",
        "CZT length + bins - 1 must be <= 8192, got 3 + 8191 - 1",
    ]

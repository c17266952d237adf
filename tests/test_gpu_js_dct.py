"""dct / idct of the JS host (pragma-dsp_amd/js `.dct`, through the N-API addon) against the f64 numpy restatement
of test_dct_cpu on seeded inputs: plain / Float64Array / Float32Array inputs, both types, every norm, the error
texts, and the root's key list, which `.dct` must not join."""
import functools

import numpy as np
import pytest

import js_host
from test_dct_cpu import NORMS, dct_ref, idct_ref

pytestmark = [pytest.mark.gpu, js_host.needs_node]
run_cases = functools.partial(js_host.run_cases, "dct_cases.js")


def test_js_dct_against_numpy(tmp_path):
    rng = np.random.default_rng(43)
    cases, want = [], []
    for n in (64, 1024, 16384):
        x = rng.standard_normal(n)
        for typed in (None, "f64", "f32"):
            xin = x.astype(np.float32).astype(np.float64) if typed == "f32" else x
            for op in ("dct", "idct"):
                for t in (None, 2, 3):
                    for norm in (None,) + NORMS:
                        cases.append({"op": op, "signal": x.tolist(), "type": t, "norm": norm, "typed": typed})
                        fn = dct_ref if op == "dct" else idct_ref
                        want.append(fn(xin, t or 2, norm or "backward"))
    got, keys = run_cases(cases, tmp_path)
    assert keys == ["spectrum", "spectrumBatch", "spectrumStream", "core", "fourier"]
    for c, g, w in zip(cases, got, want):
        assert isinstance(g, list), (c["op"], c["type"], c["norm"], g)
        g = np.asarray(g)
        assert np.abs(g - w).max() <= 1e-15 * np.log2(w.size) * np.abs(w).max(), (c["op"], c["type"], c["norm"])


def test_js_dct_errors(tmp_path):
    x = [1.0] * 256
    cases = [
        {"op": "dct", "signal": x, "type": 4, "norm": None, "typed": None},
        {"op": "idct", "signal": x, "type": 1, "norm": None, "typed": None},
        {"op": "dct", "signal": x, "type": None, "norm": "unit", "typed": None},
        {"op": "dct", "signal": [1.0] * 100, "type": None, "norm": None, "typed": None},
        {"op": "dct", "signal": [1.0] * 32, "type": 3, "norm": None, "typed": "f64"},
        {"op": "idct", "signal": [1.0] * 32768, "type": None, "norm": "ortho", "typed": "f32"},
        {"op": "dct", "signal": [], "type": None, "norm": None, "typed": None},
    ]
    got, _ = run_cases(cases, tmp_path)
    assert [g["error"] for g in got] == [
        "DCT type must be 2 or 3, got 4",
        "DCT type must be 2 or 3, got 1",
        "DCT norm must be 'backward', 'ortho' or 'forward', got unit",
        "FFT size must be power of two, got 100",
        "DCT needs a plan of 64 <= N <= 16384, got 32",
        "DCT needs a plan of 64 <= N <= 16384, got 32768",
        "FFT size must be power of two, got 0",
    ]

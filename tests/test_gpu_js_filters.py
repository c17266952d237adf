"""firFilter of the JS host (pragma-dsp_amd/js `.filters`, through the N-API addon) against numpy.convolve on
seeded inputs: every mode, plain / Float64Array / Float32Array inputs, and the error texts."""

import numpy as np
import pytest

import js_host

pytestmark = [pytest.mark.gpu, js_host.needs_node]


def run_cases(cases, tmp_path):
    return js_host.run_cases("filters_cases.js", cases, tmp_path, tail=0)[0]


def test_js_fir_filter_against_numpy(tmp_path):
    rng = np.random.default_rng(99)
    cases, want = [], []
    for length, p in ((1, 1), (4, 9), (100, 31), (5000, 256), (2000, 2048)):
        x, h = rng.standard_normal(length), rng.standard_normal(p)
        for typed in (None, "f64", "f32"):
            xq = x.astype(np.float32).astype(np.float64) if typed == "f32" else x
            hq = h.astype(np.float32).astype(np.float64) if typed == "f32" else h
            full = np.convolve(xq, hq)
            for mode in (None, "full", "same", "valid", "filter"):
                cases.append({"signal": x.tolist(), "taps": h.tolist(), "mode": mode, "typed": typed})
                ref = full[:length] if mode == "filter" else np.convolve(xq, hq, mode=mode or "full")
                want.append((ref, np.abs(xq).max() * np.abs(hq).sum()))
    cases.append({"signal": [1.0, 2.0], "taps": [1.0], "mode": "circular", "typed": None})
    cases.append({"signal": [], "taps": [1.0], "mode": None, "typed": None})
    cases.append({"signal": [1.0], "taps": [0.0] * 8193, "mode": None, "typed": None})
    res = run_cases(cases, tmp_path)
    for got, (ref, scale), c in zip(res, want, cases):
        assert not isinstance(got, dict), (got, c["mode"], c["typed"])
        got = np.array(got)
        assert got.shape == ref.shape, (len(c["signal"]), len(c["taps"]), c["mode"])
        assert np.abs(got - ref).max() / scale <= 1e-13, (len(c["signal"]), len(c["taps"]), c["mode"], c["typed"])
    assert res[-3] == {"error": "Unsupported FIR mode: circular"}
    assert res[-2]["error"].startswith("signal and filter must not be empty")
    assert "exceeds N/2 = 8192" in res[-1]["error"]

"""resamplePoly / upfirdn / designResampleTaps of the JS host (pragma-dsp_amd/js `.filters`, through the N-API addon)
against the f64 restatement of the definition in test_resample_cpu on seeded inputs, at the f64 bound of
test_gpu_resample ((T + 2) 2^-52 A[m] per output): plain / Float64Array / Float32Array inputs, default and user taps,
the error texts, and the root's key list, which `.filters` must not join."""
import functools

import numpy as np
import pytest

import js_host
import pragma_dsp_amd as pd
from test_resample_cpu import poly_setup, resample_ref, user_taps

pytestmark = [pytest.mark.gpu, js_host.needs_node]
run_cases = functools.partial(js_host.run_cases, "resample_cases.js")
EPS = 2.0 ** -52


def held(got, x, up, down, h, t0, y_len):
    got = np.asarray(got)
    assert got.shape == (y_len,)
    ref = resample_ref(x, up, down, h, t0, y_len)[0]
    a = resample_ref(x, up, down, h, t0, y_len, abs=True)[0]
    t = -(-h.size // up)
    return np.all(np.abs(got - ref) <= (t + 2) * EPS * a)


def test_js_resample_against_numpy(tmp_path):
    rng = np.random.default_rng(53)
    n = 500
    x = rng.standard_normal(n)
    w = user_taps(17)
    cases, want = [], []
    for up, down in ((3, 2), (1, 2), (160, 147)):
        for typed in ("f32", "f64", None):
            xin = x.astype(np.float32).astype(np.float64) if typed == "f32" else x
            for taps in (None, w):
                cases.append({"op": "resamplePoly", "signal": x.tolist(), "up": up, "down": down,
                              "taps": None if taps is None else taps.tolist(), "typed": typed})
                u, d, h, t0 = poly_setup(up, down, taps)
                want.append((xin, u, d, h, t0, -(-n * u // d)))
            cases.append({"op": "upfirdn", "signal": x.tolist(), "up": up, "down": down, "taps": w.tolist(), "typed": typed})
            want.append((xin, up, down, w, 0, ((n - 1) * up + 16) // down + 1))
    cases.append({"op": "upfirdn", "signal": x.tolist(), "up": None, "down": None, "taps": w.tolist(), "typed": None})
    want.append((x, 1, 1, w, 0, n + 16))
    designs = [(3, 2), (1, 2), (160, 147), (4, 6)]
    cases += [{"op": "designResampleTaps", "up": u, "down": d} for u, d in designs]
    got, keys = run_cases(cases, tmp_path)
    assert keys == ["spectrum", "spectrumBatch", "spectrumStream", "core", "fourier"]
    for c, g, wnt in zip(cases, got, want):
        assert isinstance(g, list), (c["op"], c["up"], c["down"], g)
        assert held(g, *wnt), (c["op"], c["up"], c["down"], c["typed"])
    for (u, d), g in zip(designs, got[len(want):]):
        assert np.array_equal(np.asarray(g), pd.design_taps(u, d))


def test_js_resample_errors(tmp_path):
    x = [1.0] * 64
    cases = [
        {"op": "resamplePoly", "signal": x, "up": 0, "down": 1, "taps": None, "typed": None},
        {"op": "resamplePoly", "signal": x, "up": 2, "down": -1, "taps": None, "typed": "f32"},
        {"op": "resamplePoly", "signal": x, "up": 2, "down": 1, "taps": [1.0] * 8193, "typed": None},
        {"op": "upfirdn", "signal": x, "up": 1, "down": 1, "taps": [1.0] * 8193, "typed": "f64"},
        {"op": "resamplePoly", "signal": x, "up": 8192, "down": 1, "taps": None, "typed": None},
        {"op": "designResampleTaps", "up": 8192, "down": 1},
        {"op": "resamplePoly", "signal": x, "up": 2.5, "down": 1, "taps": None, "typed": None},
        {"op": "upfirdn", "signal": x, "up": 2, "down": "1", "taps": [1.0], "typed": None},
        {"op": "resamplePoly", "signal": [], "up": 2, "down": 1, "taps": None, "typed": None},
        {"op": "upfirdn", "signal": x, "up": 2, "down": 1, "taps": [], "typed": None},
        {"op": "resamplePoly", "signal": x, "up": 2, "down": 1, "taps": [], "typed": None},
    ]
    got, _ = run_cases(cases, tmp_path)
    too_many = "the default filter for 8192/1 has 163841 taps, beyond the 8192 a resampler holds (pass shorter taps)"
    assert [g["error"] for g in got] == [
        "up and down must be >= 1, got up 0, down 1",
        "up and down must be >= 1, got up 2, down -1",
        "filter of 8193 taps exceeds the 8192 a resampler holds",
        "filter of 8193 taps exceeds the 8192 a resampler holds",
        too_many,
        too_many,
        "up must be an integer, got 2.5",
        "down must be an integer, got 1",
        "len must be >= 1, got 0",
        "filter must have at least one tap, got 0",
        "filter must have at least one tap, got 0",
    ]

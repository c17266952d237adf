"""wavedec / waverec / waveletTaps of the JS host (pragma-dsp_amd/js `.wavelet`, through the N-API addon) against the
numpy restatement of tests/test_dwt_cpu.py at the f64 bounds of test_gpu_dwt, on plain arrays, Float64Array and
Float32Array; the error texts; and the root's key list, which `.wavelet` must not join."""
import functools

import numpy as np
import pytest
import torch

import js_host
import pragma_dsp_amd as pd
from test_dwt_cpu import band_levels, lattice_taps, wavedec_ref, waverec_ref
from test_gpu_dwt import hold

pytestmark = [pytest.mark.gpu, js_host.needs_node]
run_cases = functools.partial(js_host.run_cases, "dwt_cases.js")
EPS = 2.0 ** -52


def test_js_wavelet_against_the_restatement(tmp_path):
    rng = np.random.default_rng(71)
    custom = lattice_taps(6, 72)
    cases, checks = [], []
    for n, levels, wv in ((2, 1, "haar"), (96, 5, "db2"), (4096, 12, "db10"), (4096, 6, custom), (98304, 8, "db8")):
        h = pd.wavelet_taps(wv) if isinstance(wv, str) else wv
        x = rng.standard_normal(n)
        for typed in (None, "f64", "f32"):
            xin = x.astype(np.float32).astype(np.float64) if typed == "f32" else x
            k = (h.size + 2) * EPS
            jw = wv if isinstance(wv, str) else wv.tolist()
            cases.append({"op": "wavedec", "signal": x.tolist(), "wavelet": jw, "levels": levels, "typed": typed})
            checks.append((wavedec_ref(xin, h, levels), band_levels(n, levels) * k * wavedec_ref(xin, h, levels, abs=True)))
            cases.append({"op": "waverec", "signal": x.tolist(), "wavelet": jw, "levels": levels, "typed": typed})
            checks.append((waverec_ref(xin, h, levels), levels * k * waverec_ref(xin, h, levels, abs=True)))
    names = ["haar"] + [f"db{p}" for p in range(1, 11)]
    cases += [{"op": "waveletTaps", "wavelet": nm} for nm in names]
    got, keys = run_cases(cases, tmp_path)
    assert keys == ["spectrum", "spectrumBatch", "spectrumStream", "core", "fourier"]
    for c, g, (ref, bound) in zip(cases, got, checks):
        assert isinstance(g, dict) and "values" in g, (c["op"], len(c["signal"]), g)
        hold(np.asarray(g["values"]), ref, bound, f"js {c['op']} n {len(c['signal'])} J {c['levels']} {c['typed']}")
    for nm, g in zip(names, got[len(checks):]):
        assert np.array_equal(np.asarray(g["values"]), pd.wavelet_taps(nm)), nm


def test_js_wavelet_errors(tmp_path):
    x8 = [1.0] * 8
    cases = [
        {"op": "wavedec", "signal": x8, "wavelet": "sym4", "levels": 2, "typed": None},
        {"op": "waverec", "signal": x8, "wavelet": "db2", "levels": 0, "typed": "f64"},
        {"op": "wavedec", "signal": [1.0] * 10, "wavelet": "db2", "levels": 2, "typed": "f32"},
        {"op": "wavedec", "signal": [], "wavelet": "haar", "levels": 1, "typed": None},
        {"op": "wavedec", "signal": x8, "wavelet": [0.5, 0.5, 0.5], "levels": 1, "typed": None},
        {"op": "waverec", "signal": x8, "wavelet": [0.5, 0.5], "levels": 1, "typed": None},
        {"op": "wavedec", "signal": x8, "wavelet": "db2", "levels": 1.5, "typed": None},
        {"op": "wavedec", "signal": [0.0] * (1 << 17), "wavelet": "db4", "levels": 11, "typed": "f64"},
        {"op": "waveletTaps", "wavelet": "coif1"},
    ]
    got, _ = run_cases(cases, tmp_path)
    assert [g["error"] for g in got] == [
        'unknown wavelet "sym4" (haar, db1 ... db10)',
        "levels must be >= 1, got 0",
        "len must be a positive multiple of 2^levels (levels = 2), got 10",
        "len must be a positive multiple of 2^levels (levels = 1), got 0",
        "the scaling filter must have an even number of taps, 2 ... 32, got 3",
        "the taps are not an orthonormal scaling filter: sum_k h[k] h[k + 0] is not 1 within 1e-10",
        "levels must be an integer",
        "forward DWT of 11 levels with 8 taps on rows of 131072: beyond the resident path max(halo, 2^levels) must be "
        "<= 4096 values, halo = (taps - 2)(2^levels - 1): at most 9 levels",
        'unknown wavelet "coif1" (haar, db1 ... db10)',
    ]

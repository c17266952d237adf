"""hilbert / envelope / instantaneousPhase of the JS host (pragma-dsp_amd/js `.hilbert`, through the N-API addon)
against the f64 numpy restatement of test_hilbert_cpu on seeded inputs, at the f64 bound of test_gpu_hilbert: plain /
Float64Array / Float32Array inputs, with and without padding, the error texts, and the root's key list, which
`.hilbert` must not join."""
import functools

import numpy as np
import pytest

import js_host
from test_gpu_hilbert import bound, err_rows
from test_hilbert_cpu import hilbert_ref

pytestmark = [pytest.mark.gpu, js_host.needs_node]
run_cases = functools.partial(js_host.run_cases, "hilbert_cases.js")
OPS = {"hilbert": "analytic", "envelope": "envelope", "instantaneousPhase": "phase"}


def test_js_hilbert_against_numpy(tmp_path):
    rng = np.random.default_rng(47)
    cases, want = [], []
    for n in (64, 1024, 16384):
        x = rng.standard_normal(n)
        for typed in (None, "f64", "f32"):
            xin = x.astype(np.float32).astype(np.float64) if typed == "f32" else x
            for op in OPS:
                for ln, nopt in ((n, None), (n, n), (n // 2 + 1, n), (1, n)):
                    cases.append({"op": op, "signal": x[:ln].tolist(), "n": nopt, "typed": typed})
                    want.append((n, hilbert_ref(xin[:ln], n)))
    got, keys = run_cases(cases, tmp_path)
    assert keys == ["spectrum", "spectrumBatch", "spectrumStream", "core", "fourier"]
    for c, g, (n, a_ref) in zip(cases, got, want):
        mode = OPS[c["op"]]
        if mode == "analytic":
            assert isinstance(g, dict) and "real" in g, (c["op"], c["n"], g)
            g = np.asarray(g["real"]) + 1j * np.asarray(g["imag"])
            assert np.array_equal(g.real, a_ref.real)  # the zero-padded signal itself
        else:
            assert isinstance(g, list), (c["op"], c["n"], g)
            g = np.asarray(g)
        assert g.shape == (n,)
        assert err_rows(g, a_ref, mode) <= bound("f64", n, mode), (c["op"], c["n"], c["typed"])


def test_js_hilbert_errors(tmp_path):
    x = [1.0] * 256
    cases = [
        {"op": "hilbert", "signal": [1.0] * 100, "n": None, "typed": None},
        {"op": "envelope", "signal": x, "n": 1000, "typed": None},
        {"op": "instantaneousPhase", "signal": [1.0] * 32, "n": None, "typed": "f64"},
        {"op": "hilbert", "signal": x, "n": 32768, "typed": "f32"},
        {"op": "envelope", "signal": x, "n": 128, "typed": None},
        {"op": "hilbert", "signal": [], "n": None, "typed": None},
        {"op": "hilbert", "signal": [], "n": 64, "typed": None},
        {"op": "envelope", "signal": x, "n": 256.5, "typed": None},
        {"op": "instantaneousPhase", "signal": x, "n": "256", "typed": None},
    ]
    got, _ = run_cases(cases, tmp_path)
    assert [g["error"] for g in got] == [
        "FFT size must be power of two, got 100",
        "FFT size must be power of two, got 1000",
        "the Hilbert transform needs a plan of 64 <= N <= 16384, got 32",
        "the Hilbert transform needs a plan of 64 <= N <= 16384, got 32768",
        "len must be 1 ... N = 128, got 256",
        "FFT size must be power of two, got 0",
        "len must be 1 ... N = 64, got 0",
        "n must be an integer, got 256.5",
        "n must be an integer, got 256",
    ]

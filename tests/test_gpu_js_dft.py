"""dft / idft of the JS host (pragma-dsp_amd/js `.dft`, through the N-API addon) against numpy.fft.fft / ifft on seeded
inputs at the f64 bound of test_gpu_dft: L = 3, 1000 and 4095, plain / Float64Array / Float32Array inputs, real and
complex, the error texts, and the root's key list, which `.dft` must not join."""
import functools

import numpy as np
import pytest

import js_host
from test_dft_cpu import row_err
from test_gpu_dft import bound

pytestmark = [pytest.mark.gpu, js_host.needs_node]
run_cases = functools.partial(js_host.run_cases, "dft_cases.js")


def test_js_dft_against_numpy(tmp_path):
    rng = np.random.default_rng(53)
    cases, want = [], []
    for ln in (3, 1000, 4095):
        z = rng.standard_normal(ln) + 1j * rng.standard_normal(ln)
        for typed in (None, "f64", "f32"):
            zin = z.astype(np.complex64).astype(np.complex128) if typed == "f32" else z
            cases.append({"op": "dft", "real": z.real.tolist(), "imag": z.imag.tolist(), "typed": typed})
            want.append(np.fft.fft(zin))
            cases.append({"op": "dft", "real": z.real.tolist(), "imag": None, "typed": typed})
            want.append(np.fft.fft(zin.real))
            cases.append({"op": "idft", "real": z.real.tolist(), "imag": z.imag.tolist(), "typed": typed})
            want.append(np.fft.ifft(zin))
    got, keys = run_cases(cases, tmp_path)
    assert keys == ["spectrum", "spectrumBatch", "spectrumStream", "core", "fourier"]
    for c, g, w in zip(cases, got, want):
        assert isinstance(g, dict) and "real" in g, (c["op"], len(c["real"]), g)
        g = np.asarray(g["real"]) + 1j * np.asarray(g["imag"])
        assert g.shape == w.shape
        assert row_err(g, w) <= bound("f64", len(w)), (c["op"], len(w), c["typed"])


def test_js_dft_errors(tmp_path):
    cases = [
        {"op": "dft", "real": [1.0] * 4097, "imag": None, "typed": None},
        {"op": "idft", "real": [1.0] * 4097, "imag": [0.0] * 4097, "typed": "f64"},
        {"op": "dft", "real": [1.0], "imag": None, "typed": None},
        {"op": "dft", "real": [], "imag": None, "typed": "f32"},
        {"op": "dft", "real": [1.0, 2.0, 3.0], "imag": [1.0, 2.0], "typed": None},
        {"op": "idft", "real": [1.0, 2.0, 3.0], "imag": None, "typed": None},
    ]
    got, _ = run_cases(cases, tmp_path)
    assert [g["error"] for g in got] == [
        "DFT length must be 2 ... 4096, got 4097",
        "DFT length must be 2 ... 4096, got 4097",
        "DFT length must be 2 ... 4096, got 1",
        "DFT length must be 2 ... 4096, got 0",
        "real and imag must have the same length, got 3 and 2",
        "imag must be an array or a typed array",
    ]

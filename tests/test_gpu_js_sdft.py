"""slidingDft / goertzel of the JS host (pragma-dsp_amd/js `.sdft`, through the N-API addon) against the Python host
form (the same f64 kernel: the bits agree) and the long double direct sum: plain / Float64Array / Float32Array inputs,
the defaults, every window, the error texts, and the root's key list, which `.sdft` must not join."""
import functools

import numpy as np
import pytest

import js_host
import sdft_ref as R

pytestmark = [pytest.mark.gpu, js_host.needs_node]
run_cases = functools.partial(js_host.run_cases, "sdft_cases.js")


def test_js_sdft_against_the_python_host_form(pdsp, tmp_path):
    rng = np.random.default_rng(67)
    cases, want = [], []
    for n, hop, length, bins in ((64, 1, 300, [0, 3, 12.5]), (100, 7, 1000, [-3, 12.5, 102]), (1000, 250, 5000, [250]),
                                 (4096, 1024, 9000, [0.25, 2048])):
        x = rng.standard_normal(length)
        for kind in (None, "rect", "hann", "hamming", "blackman"):
            for typed in (None, "f64", "f32"):
                xq = x.astype(np.float32).astype(np.float64) if typed == "f32" else x
                cases.append({"op": "slidingDft", "signal": x.tolist(), "size": n, "bins": bins, "hop": hop,
                              "window": kind, "typed": typed})
                want.append((pdsp.sliding_dft(xq, n, bins, hop, kind or "rect"), xq, n, hop, bins, kind or "rect"))
        cases.append({"op": "goertzel", "signal": x[:n].tolist(), "size": None, "bins": bins, "hop": None,
                      "window": None, "typed": None})
        want.append((pdsp.goertzel(x[:n], bins), x[:n], n, 1, bins, "rect"))
    # the defaults: hop 1, rectangular; one bin as a number
    x = rng.standard_normal(200)
    cases.append({"op": "slidingDft", "signal": x.tolist(), "size": 50, "bins": 4.5, "hop": None, "window": None,
                  "typed": None})
    want.append((pdsp.sliding_dft(x, 50, 4.5), x, 50, 1, [4.5], "rect"))
    got, keys = run_cases(cases, tmp_path)
    assert keys == ["spectrum", "spectrumBatch", "spectrumStream", "core", "fourier"]
    for c, g, (w, x, n, hop, bins, win) in zip(cases, got, want):
        assert isinstance(g, dict) and "real" in g, (c["op"], c["size"], g)
        z = np.asarray(g["real"]) + 1j * np.asarray(g["imag"])
        if c["op"] == "slidingDft":
            assert (g["bins"], g["frames"]) == w.shape
        assert np.array_equal(z.reshape(w.shape), w), (c["op"], n, win, c["typed"])
        dre, dim = R.direct(x, n, bins, hop, win)
        assert R.err_units(w.reshape(dre.shape), dre, dim, n, "f64", np.abs(x).max()) <= R.BOUND["f64"]


def test_js_sdft_errors(tmp_path):
    one = {"op": "slidingDft", "signal": [1.0] * 100, "size": 64, "bins": [1.0], "hop": 1, "window": None, "typed": None}
    cases = [
        dict(one, size=1),
        dict(one, size=20000),
        dict(one, size=64.5),
        dict(one, hop=0),
        dict(one, hop=2.5),
        dict(one, window="kaiser"),
        dict(one, bins=[]),
        dict(one, bins=[0.0] * 257),
        dict(one, bins="x"),
        dict(one, signal=[1.0] * 10),
        dict(one, op="goertzel", signal=[1.0], bins=[0.0]),
    ]
    got, _ = run_cases(cases, tmp_path)
    assert [g["error"] for g in got] == [
        "sliding DFT window length must be 2 ... 16384, got 1",
        "sliding DFT window length must be 2 ... 16384, got 20000",
        "size must be an integer, got 64.5",
        "hop must be >= 1, got 0",
        "hop must be an integer, got 2.5",
        "Unsupported window type: kaiser",
        "sliding DFT bins must be 1 ... 256, got 0",
        "sliding DFT bins must be 1 ... 256, got 257",
        "bins must be an array or a typed array",
        "sliding DFT rows of 10 samples are shorter than the window of 64",
        "sliding DFT window length must be 2 ... 16384, got 1",
    ]

"""stft / istft of the JS host (pragma-dsp_amd/js `.stft`, through the N-API addon) against numpy on seeded inputs:
plain / Float64Array / Float32Array inputs, every window type, and the error texts."""

import numpy as np
import pytest

import js_host

pytestmark = [pytest.mark.gpu, js_host.needs_node]


def run_cases(cases, tmp_path):
    return js_host.run_cases("stft_cases.js", cases, tmp_path, tail=0)[0]


def window(kind, n):
    from pragma_dsp_amd import createWindow
    return createWindow(kind, n)


def ref_istft(z, n, hop, w):
    z = z.copy()
    z[:, 0] = z[:, 0].real
    z[:, -1] = z[:, -1].real
    y = np.fft.irfft(z, n, axis=1)
    total = (z.shape[0] - 1) * hop + n
    num, den = np.zeros(total), np.zeros(total)
    for b in range(z.shape[0]):
        num[b * hop:b * hop + n] += w * y[b]
        den[b * hop:b * hop + n] += w * w
    return np.where(den > 1e-11, num / np.where(den > 1e-11, den, 1.0), 0.0), den


def test_js_stft_pair_against_numpy(tmp_path):
    rng = np.random.default_rng(41)
    cases, want = [], []
    for n, hop, length in ((64, 16, 300), (256, 256, 1000), (1024, 300, 5000), (4096, 1024, 9000)):
        x = rng.standard_normal(length)
        frames = 1 + (length - n) // hop
        z = rng.standard_normal((frames, n // 2 + 1)) + 1j * rng.standard_normal((frames, n // 2 + 1))
        for kind in (None, "rect", "hann", "hamming", "blackman"):
            w = window(kind or "hann", n)
            for typed in (None, "f64", "f32"):
                xq = x.astype(np.float32).astype(np.float64) if typed == "f32" else x
                idx = np.arange(frames)[:, None] * hop + np.arange(n)[None, :]
                cases.append({"op": "stft", "signal": x.tolist(), "fftSize": n, "hopSize": hop, "window": kind, "typed": typed})
                want.append(("stft", np.fft.rfft(xq[idx] * w, axis=1), None))
                zq = (z.real.astype(np.float32) + 1j * z.imag.astype(np.float32)).astype(np.complex128) if typed == "f32" else z
                cases.append({"op": "istft", "frames": frames, "real": z.real.reshape(-1).tolist(),
                              "imag": z.imag.reshape(-1).tolist(), "fftSize": n, "hopSize": hop, "window": kind,
                              "typed": typed})
                want.append(("istft",) + ref_istft(zq, n, hop, w))
    errors = [
        ({"op": "stft", "signal": [1.0] * 10, "fftSize": 64, "hopSize": 8, "window": None, "typed": None},
         "signal length 10 is shorter than one frame (64)"),
        ({"op": "stft", "signal": [1.0] * 100, "fftSize": 48, "hopSize": 8, "window": None, "typed": None},
         "FFT size must be power of two, got 48"),
        ({"op": "stft", "signal": [1.0] * 100, "fftSize": 64, "hopSize": 8, "window": "kaiser", "typed": None},
         "Unsupported window type: kaiser"),
        ({"op": "istft", "frames": 2, "real": [0.0] * 66, "imag": [0.0] * 66, "fftSize": 64, "hopSize": 0,
          "window": None, "typed": None}, "hop must be >= 1, got 0"),
        ({"op": "istft", "frames": 2, "real": [0.0] * 65, "imag": [0.0] * 66, "fftSize": 64, "hopSize": 8,
          "window": None, "typed": None}, "real and imag must hold frames * (fftSize/2 + 1) = 66 values, got 65 and 66"),
    ]
    res = run_cases(cases + [c for c, _ in errors], tmp_path)
    for got, (op, ref, den), c in zip(res, want, cases):
        assert "error" not in got, (got, c["fftSize"], c["window"])
        if op == "stft":
            assert got["frames"] == ref.shape[0] and got["bins"] == ref.shape[1]
            g = np.array(got["real"]).reshape(ref.shape) + 1j * np.array(got["imag"]).reshape(ref.shape)
            assert np.abs(g - ref).max() <= 1e-14 * np.abs(ref).max(), (c["fftSize"], c["window"], c["typed"])
        else:
            g = np.array(got)
            assert g.shape == ref.shape
            good = den >= 1e-3 * den.max()
            assert np.abs(g - ref)[good].max() <= 1e-13 * np.abs(ref).max(), (c["fftSize"], c["window"], c["typed"])
            assert np.all(g[den <= 1e-11] == 0.0)
    for got, (_, text) in zip(res[len(cases):], errors):
        assert got == {"error": text}

"""Short-time Fourier transform with complex output and its weighted overlap-add inverse -- the reference's
roadmap "A) STFT" (ROADMAP.md: pragma-dsp/xform/stft, stft(signal, opts) with complex output) and the way back to
the time domain -- as host f64 forms (numpy in, numpy out) through pdsp_stft_host_f64 / pdsp_istft_host_f64.

    stft(signal, fftSize, hopSize, window="hann")  -> complex128 [F, fftSize/2 + 1], F = 1 + (len - fftSize) // hopSize
    istft(spec, hopSize, window="hann")            -> float64 [(F - 1) * hopSize + fftSize]

Frame b is signal[b*hop : b*hop + N]; its bins are the one-sided DFT of w * frame, unscaled.  The inverse is
out[t] = sum_b w[t - b h] y_b[t - b h] / sum_b w[t - b h]^2 with y_b the inverse real DFT of X_b (1/N), and 0 where the
denominator is <= 1e-11: torch.istft(center=False) wherever its NOLA check passes.  64 <= N <= 16384.  The device
forms are BatchedFft.stft_complex / BatchedFft.istft (batch.py).
"""
from __future__ import annotations

import numpy as np

from . import _capi
from ._capi import PdspError, check, lib


def _window_type(window) -> int:
    if window not in _capi.WINDOW_TYPES:
        raise PdspError(_capi.ERR_WINDOW_TYPE, f"Unsupported window type: {window}")
    return _capi.WINDOW_TYPES[window]


def stft(signal, fftSize: int, hopSize: int, window: str = "hann") -> np.ndarray:  # noqa: N803 (reference names)
    """Complex bins [frames, fftSize/2 + 1] of the frames of a 1-D signal, computed on the device in f64."""
    x = np.ascontiguousarray(np.asarray(signal, dtype=np.float64))
    if x.ndim != 1:
        raise PdspError(_capi.ERR_BAD_ARG, f"signal must be 1-D, got shape {x.shape}")
    n, hop = int(fftSize), int(hopSize)
    wt = _window_type(window)
    ok = 64 <= n <= 16384 and hop >= 1 and x.size >= n  # else the library refuses before touching the outputs
    frames = 1 + (x.size - n) // hop if ok else 1
    bins = n // 2 + 1 if ok else 1
    re = np.empty((frames, bins), dtype=np.float64)
    im = np.empty((frames, bins), dtype=np.float64)
    check(lib.pdsp_stft_host_f64(_capi.dptr(x), x.size, n, hop, wt, _capi.dptr(re), _capi.dptr(im)))
    return re + 1j * im


def istft(spec, hopSize: int, window: str = "hann") -> np.ndarray:  # noqa: N803 (reference names)
    """Weighted overlap-add inverse of complex bins [frames, N/2 + 1] (N = 2 * (bins - 1)), on the device in f64."""
    z = np.asarray(spec)
    if z.ndim != 2 or z.shape[0] < 1 or z.shape[1] < 2:
        raise PdspError(_capi.ERR_BAD_ARG, f"spec must be [frames >= 1, bins >= 2], got shape {z.shape}")
    frames, bins = z.shape
    n, hop = 2 * (bins - 1), int(hopSize)
    wt = _window_type(window)
    re = np.ascontiguousarray(z.real, dtype=np.float64)
    im = np.ascontiguousarray(z.imag if np.iscomplexobj(z) else np.zeros_like(re), dtype=np.float64)
    total = (frames - 1) * hop + n
    ok = 64 <= n <= 16384 and hop >= 1 and total <= (1 << 40)  # else the library refuses before touching `out`
    out = np.empty(total if ok else 1, dtype=np.float64)
    check(lib.pdsp_istft_host_f64(_capi.dptr(re), _capi.dptr(im), frames, n, hop, wt, _capi.dptr(out)))
    return out

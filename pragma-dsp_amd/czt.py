"""The chirp-z transform and the zoom FFT of rows -- scipy.signal.czt / zoom_fft along the last axis -- one launch per
call (include/pdsp_hip.h, "chirp-z transform"): K points of the z-transform of a row of L samples on an arc of a circle,

    X[k] = sum_{n < L} x[n] a^-n w^(n k),  k < K,   w = exp(-2 pi i step),  a = radius exp(2 pi i start)

with L, K >= 1 and L + K - 1 <= 8192.  step and start are f64 numbers of TURNS, not a complex w: the tables are the
precision budget, and their phases are formed exactly from the doubles given (step = 1.0 / 1000 is the double nearest
1/1000, not 1/1000; Dft is the way to the exact L-th roots of unity).  Only arcs are built, |w| = 1; there is no inverse.

    Czt(length, bins, step, start=0.0, radius=1.0, device=None)   the tables of one transform on one GPU (f32 and f64)
      .forward(re, im=None, out=None)                             torch planes [rows, L] -> (re, im) of [rows, K]
    Czt.zoom(length, fn, bins=None, fs=2.0, endpoint=False)       the band fn = [f1, f2] (a scalar: [0, fn]) of zoom_fft
    czt(x, m=None, w=None, a=1+0j) / zoom_fft(x, fn, m=None, fs=2.0, endpoint=False)
                                    host f64 forms: numpy in (real or complex, [L] or [..., L]), complex128 out
    czt_points(m, step, start=0.0, radius=1.0)                    the K points a w^-k

torch is used for device memory and streams only; the arithmetic is the HIP kernel behind the C ABI.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _capi
from ._capi import PdspError, lib
from ._chirp import ChirpRows, host_call, host_planes
from ._chirp import integer as _int

MAX_CONV = 8192
SPIRAL = "spirals are not supported: |w| must be 1 (an arc of a circle), got |w| = {!r}"


def _real(v, name) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise PdspError(_capi.ERR_BAD_ARG, f"{name} must be a real number, got {v!r}")
    return float(v)


def _turns(n, t, mod):
    """(n t) mod `mod` in turns as (r, e), r + e exact: n integers below 2^26, t a double.  p + e is the product
    without error (Dekker's split of t stands in for the fma of the C side), fmod of p is exact, and e is added after
    the reduction."""
    n = np.asarray(n, dtype=np.float64)
    p = n * t
    c = 134217729.0 * t  # 2^27 + 1
    hi = c - (c - t)
    lo = t - hi
    e = (n * hi - p) + n * lo
    return np.fmod(p, mod), e


def czt_points(m, step, start=0.0, radius=1.0) -> np.ndarray:
    """The m points a w^-k = radius exp(2 pi i (start + k step)) the transform is evaluated at, with the phase
    reduction of the tables: complex128."""
    m, step, start, radius = _int(m, "m"), _real(step, "step"), _real(start, "start"), _real(radius, "radius")
    if m < 1:
        raise PdspError(_capi.ERR_UNSUPPORTED_SIZE, f"CZT bins must be >= 1, got {m}")
    r, e = _turns(np.arange(m), step, 1.0)
    pi = 4 * np.arctan(np.longdouble(1))
    ang = 2 * pi * ((r.astype(np.longdouble) + e) + np.longdouble(math.fmod(start, 1.0)))
    return (radius * (np.cos(ang) + 1j * np.sin(ang))).astype(np.complex128)


def _zoom(fn, bins, fs, endpoint):
    """(step, start) of zoom_fft's band."""
    f = np.asarray(fn, dtype=np.float64)
    if f.ndim == 0:
        f1, f2 = 0.0, float(f)
    elif f.shape == (2,):
        f1, f2 = float(f[0]), float(f[1])
    else:
        raise PdspError(_capi.ERR_BAD_ARG, "fn must be a scalar or a pair [f1, f2]")
    fs = _real(fs, "fs")
    if bins < 1:
        raise PdspError(_capi.ERR_UNSUPPORTED_SIZE, f"CZT bins must be >= 1, got {bins}")
    div = fs * (bins - 1 if endpoint else bins)
    if not math.isfinite(fs) or fs == 0.0 or (div == 0.0 and f2 != f1):
        raise PdspError(_capi.ERR_BAD_ARG, f"fs must be finite and non-zero (and bins > 1 with endpoint), got {fs!r}")
    return ((f2 - f1) / div if div else 0.0), f1 / fs


class Czt(ChirpRows):
    """A pdsp_czt on one GPU: the pre, post and chirp-filter tables of one transform, both precisions."""

    _destroy = lib.pdsp_czt_destroy

    def _entry(self, sfx):
        return getattr(lib, "pdsp_czt_" + sfx)

    def __init__(self, length, bins, step, start=0.0, radius=1.0, device=None):
        length, bins = _int(length, "length"), _int(bins, "bins")
        step, start, radius = _real(step, "step"), _real(start, "start"), _real(radius, "radius")
        self._create(lib.pdsp_czt_create, device, length, bins, step, start, radius)
        self.length = int(lib.pdsp_czt_length(self._h))
        self.bins = int(lib.pdsp_czt_bins(self._h))
        self.conv_size = int(lib.pdsp_czt_conv_size(self._h))  # M, the points of the circular convolution
        self.step, self.start, self.radius = step, start, radius

    @classmethod
    def zoom(cls, length, fn, bins=None, fs=2.0, endpoint=False, device=None):
        """scipy.signal.ZoomFFT's parameters: the band fn = [f1, f2] (a scalar: [0, fn]) of a signal sampled at fs, in
        `bins` points (default: length); step = (f2 - f1) / (fs (bins - 1 if endpoint else bins)), start = f1 / fs."""
        length = _int(length, "length")
        bins = length if bins is None else _int(bins, "bins")
        step, start = _zoom(fn, bins, fs, endpoint)
        return cls(length, bins, step, start, 1.0, device)

    def forward(self, re: torch.Tensor, im: torch.Tensor | None = None, out=None):
        """Rows along the last axis ([..., L] contiguous, or a 2-D view with a row stride >= L) -> (re, im) of
        [..., K]; im None means real rows.  One launch on the current stream.  out: a pair of planes [..., K]; the
        exact in-place call out=(re, im) is taken where the row strides are equal."""
        return self._run(re, im, out)


def _host(x, bins, step, start, radius) -> np.ndarray:
    a, re, im = host_planes(x)
    ln = a.shape[-1]
    bins = ln if bins is None else _int(bins, "m")
    return host_call(lib.pdsp_czt_host_f64, a, re, im, bins, ln >= 1 and bins >= 1 and ln + bins - 1 <= MAX_CONV,
                     bins, step, start, radius)


def czt(x, m=None, w=None, a=1 + 0j) -> np.ndarray:
    """scipy.signal.czt along the last axis, computed on the device in f64: m points (default: len) from a in steps of
    w -- None: exp(-2 pi i / m), the DFT's; a complex w must lie on the unit circle (||w| - 1| <= 4 eps: its angle
    becomes step), else the spiral error.  complex128 [..., m]."""
    if m is None:
        m = np.asarray(x).shape[-1] if np.asarray(x).ndim else 0
    m = _int(m, "m")
    if w is None:
        step = 1.0 / m if m >= 1 else 0.0
    else:
        w = complex(w)
        if not abs(abs(w) - 1.0) <= 4 * np.finfo(np.float64).eps:
            raise PdspError(_capi.ERR_BAD_ARG, SPIRAL.format(abs(w)))
        step = -math.atan2(w.imag, w.real) / (2 * math.pi)
    a = complex(a)
    return _host(x, m, step, math.atan2(a.imag, a.real) / (2 * math.pi), abs(a))


def zoom_fft(x, fn, m=None, fs=2.0, endpoint=False) -> np.ndarray:
    """scipy.signal.zoom_fft along the last axis, computed on the device in f64: m points (default: len) of the band
    fn = [f1, f2] (a scalar: [0, fn]) of a signal sampled at fs.  complex128 [..., m]."""
    if m is None:
        m = np.asarray(x).shape[-1] if np.asarray(x).ndim else 0
    m = _int(m, "m")
    step, start = _zoom(fn, m, fs, endpoint)
    return _host(x, m, step, start, 1.0)

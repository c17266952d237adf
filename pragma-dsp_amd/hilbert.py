"""Hilbert transform helpers -- the reference's roadmap v0.3 ("Hilbert / analytic signal helpers") -- as host f64
forms (numpy in, numpy out) through pdsp_hilbert_host_f64.

    hilbert(x, n=None)              -> scipy.signal.hilbert(x, N=n) along the last axis (complex128)
    envelope(x, n=None)             -> abs(hilbert(x, n))
    instantaneous_phase(x, n=None)  -> angle(hilbert(x, n)), in (-pi, pi], not unwrapped

x is 1-D or 2-D (rows along the last axis) of len values; n, a power of two with 64 <= n <= 16384 and n >= len, is the
length each row is zero-padded to and the length of every output row.  n None means len, which must then be such a
power of two.  The device forms are BatchedFft.hilbert / hilbert_imag / envelope / instantaneous_phase (batch.py).
"""
from __future__ import annotations

import numpy as np

from . import _capi
from ._capi import PdspError, check, lib
from ._device import host_rows, integer


def _run(x, n, mode: str) -> np.ndarray:
    a, a2 = host_rows(x, "x")
    if a.ndim > 2 or a.shape[-1] == 0:
        raise PdspError(_capi.ERR_BAD_ARG, f"x must be 1-D or 2-D with rows along the last axis, got shape {a.shape}")
    rows, ln = a2.shape
    n = ln if n is None else integer(n, "n")
    k = 2 if mode == "analytic" else 1
    # a size the library refuses gets no buffer: the library fails before it writes
    y = np.empty(a.shape[:-1] + ((n if 64 <= n <= 16384 else 0) * k,), dtype=np.float64)
    check(lib.pdsp_hilbert_host_f64(_capi.dptr(a2), rows, ln, n, _capi.HILBERT_OUT[mode], _capi.dptr(y)))
    return y


def hilbert(x, n: int | None = None) -> np.ndarray:
    """scipy.signal.hilbert(x, N=n, axis=-1) computed on the device in f64: x + i Hx, complex128."""
    return _run(x, n, "analytic").view(np.complex128)


def envelope(x, n: int | None = None) -> np.ndarray:
    """abs(scipy.signal.hilbert(x, N=n, axis=-1)) computed on the device in f64."""
    return _run(x, n, "envelope")


def instantaneous_phase(x, n: int | None = None) -> np.ndarray:
    """angle(scipy.signal.hilbert(x, N=n, axis=-1)) computed on the device in f64."""
    return _run(x, n, "phase")

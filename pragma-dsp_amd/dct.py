"""Discrete cosine transform, types 2 and 3 -- the reference's roadmap v0.3 (ROADMAP.md: pragma-dsp/xform/dct,
dct(signal, { type }), idct(...)) -- as host f64 forms (numpy in, numpy out) through pdsp_dct_host_f64.

    dct(x, type=2, norm=None)   -> scipy dct(x, type, norm=norm) along the last axis
    idct(x, type=2, norm=None)  -> scipy idct(x, type, norm=norm) along the last axis

x is 1-D or 2-D (rows along the last axis) of N values, N a power of two with 64 <= N <= 16384; norm None means
"backward", as in scipy.  idct of type t and norm n is the dct of type 5 - t with "backward" and "forward" exchanged.
The device form is BatchedFft.dct / BatchedFft.idct (batch.py).
"""
from __future__ import annotations

import numpy as np

from . import _capi
from ._capi import PdspError, check, lib
from ._device import host_rows

_SWAP = {"backward": "forward", "ortho": "ortho", "forward": "backward"}


def _norm(norm) -> str:
    n = "backward" if norm is None else norm
    if n not in _capi.DCT_NORMS:
        raise PdspError(_capi.ERR_BAD_ARG, f"DCT norm must be 'backward', 'ortho' or 'forward', got {norm!r}")
    return n


def _run(x, type: int, norm: str) -> np.ndarray:
    a, a2 = host_rows(x, "x")
    if a.ndim > 2 or a.shape[-1] == 0:
        raise PdspError(_capi.ERR_BAD_ARG, f"x must be 1-D or 2-D with rows along the last axis, got shape {a.shape}")
    y = np.empty_like(a)
    check(lib.pdsp_dct_host_f64(_capi.dptr(a2), a2.shape[0], a2.shape[1], int(type), _capi.DCT_NORMS[norm], _capi.dptr(y)))
    return y


def dct(x, type: int = 2, norm: str | None = None) -> np.ndarray:
    """scipy dct(x, type, norm=norm, axis=-1) computed on the device in f64 (types 2 and 3)."""
    return _run(x, type, _norm(norm))


def idct(x, type: int = 2, norm: str | None = None) -> np.ndarray:
    """scipy idct(x, type, norm=norm, axis=-1) computed on the device in f64 (types 2 and 3)."""
    if type not in (2, 3):
        raise PdspError(_capi.ERR_BAD_ARG, f"DCT type must be 2 or 3, got {type}")
    return _run(x, 5 - type, _SWAP[_norm(norm)])

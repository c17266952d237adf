"""The multi-level discrete wavelet transform on the device: orthogonal wavelets, periodic extension, one launch per
call (include/pdsp_hip.h, "multi-level discrete wavelet transform").  The reference's roadmap lists wavelets as item E
("start with Haar + a small Daubechies set; forward/inverse DWT, multi-level decomposition") and has no such code yet,
so the definition is this library's own.  With h the scaling filter of even length F and g[j] = (-1)^j h[F - 1 - j],
one level on a row a of even length m is

    cA[k] = sum_j h[j] a[(2k + j) mod m]        cD[k] = sum_j g[j] a[(2k + j) mod m]        0 <= k < m / 2

and the inverse is its transpose.  J levels turn a row of n samples (n a multiple of 2^J) into n coefficients in the
Mallat layout [cA_J | cD_J | cD_{J-1} | ... | cD_1].

    Dwt(wavelet, levels, device=None, dtype=torch.float32)      .forward(x) / .inverse(c) / .split(c) / .max_levels(n)
    wavedec(x, wavelet, levels) / waverec(c, wavelet, levels)   one-shot device forms
    wavedecHost(signal, wavelet, levels) / waverecHost(...)     host f64 forms, numpy in / numpy out
    wavelet_taps(name)                                          "haar", "db1" ... "db10": the scaling filter, numpy f64

`wavelet` is one of those names or an array of taps (even length 2 ... 32, orthonormal to 1e-10).
torch is used for device memory and streams only; the arithmetic is the HIP kernel behind the C ABI.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _capi, _device
from ._capi import PdspError, check, lib
from ._device import host_rows, integer

MAX_TAPS = 32


def _wavelet(wavelet):
    """(name bytes or None, taps array or None, ntaps) as the C ABI takes them."""
    if isinstance(wavelet, str):
        return wavelet.encode("utf-8"), None, 0
    if isinstance(wavelet, torch.Tensor):
        wavelet = wavelet.detach().cpu().numpy()
    h = np.ascontiguousarray(np.asarray(wavelet, dtype=np.float64).reshape(-1))
    return None, h, h.size


def wavelet_taps(name: str) -> np.ndarray:
    """The scaling filter of a built-in wavelet: "haar" (= "db1"), "db2" ... "db10" (extremal phase, sum sqrt 2)."""
    if not isinstance(name, str):
        raise PdspError(_capi.ERR_BAD_ARG, f"wavelet name must be a string, got {name!r}")
    n = C.c_longlong()
    check(lib.pdsp_wavelet_taps(name.encode("utf-8"), None, C.byref(n)))
    h = np.empty(n.value, dtype=np.float64)
    check(lib.pdsp_wavelet_taps(name.encode("utf-8"), _capi.dptr(h), C.byref(n)))
    return h


class Dwt(_device.Handle):
    """A pdsp_dwt on one GPU: `levels` levels of one orthogonal wavelet over rows along the last axis."""

    _destroy = lib.pdsp_dwt_destroy

    def __init__(self, wavelet, levels, device=None, dtype=torch.float32):
        _device.suffix(dtype)
        name, h, ntaps = _wavelet(wavelet)
        levels = integer(levels, "levels", 32)
        self._open(lambda dev, out: lib.pdsp_dwt_create(dev, name, _capi.dptr(h), ntaps, levels, out), device, dtype)
        self.levels = int(lib.pdsp_dwt_levels(self._h))
        self.ntaps = int(lib.pdsp_dwt_ntaps(self._h))
        self.taps = np.empty(self.ntaps, dtype=np.float64)
        check(lib.pdsp_dwt_taps(self._h, _capi.dptr(self.taps)))

    def max_levels(self, length: int) -> int:
        """The deepest forward transform of rows of `length` values in this precision (0: none)."""
        return int(lib.pdsp_dwt_max_levels(self.ntaps, int(length), 4 if self.dtype == torch.float32 else 8))

    def _run(self, direction: str, x: torch.Tensor, out: torch.Tensor | None) -> torch.Tensor:
        _device.operand(x, "input", self.device, self.dtype, layout="rows")
        return _device.launch_rows(getattr(lib, f"pdsp_dwt_{direction}_{self._sfx}"), self._h, self, x, out,
                                   x.shape[-1] if x.dim() else 0)

    def forward(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """Rows of samples ([..., n], contiguous or a 2-D view with a row stride) -> rows of n coefficients,
        [cA_J | cD_J | ... | cD_1].  out may be x itself where the row runs in one workgroup's LDS."""
        return self._run("forward", x, out)

    def inverse(self, c: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """Rows of coefficients in forward()'s layout -> rows of samples."""
        return self._run("inverse", c, out)

    __call__ = forward

    def split(self, c):
        """Views [cA_J, cD_J, ..., cD_1] of rows of coefficients (a tensor or an array, last axis n)."""
        n = c.shape[-1]
        if n < 1 or n % (1 << self.levels):
            raise PdspError(_capi.ERR_BAD_ARG,
                            f"len must be a positive multiple of 2^levels (levels = {self.levels}), got {n}")
        m = n >> self.levels
        bands = [c[..., :m]]
        for _ in range(self.levels):
            bands.append(c[..., m:2 * m])
            m *= 2
        return bands


def wavedec(x: torch.Tensor, wavelet, levels) -> torch.Tensor:
    """One-shot device form: Dwt(wavelet, levels, x.device, x.dtype).forward(x)."""
    return Dwt(wavelet, levels, x.device, x.dtype).forward(x)


def waverec(c: torch.Tensor, wavelet, levels) -> torch.Tensor:
    """One-shot device form: Dwt(wavelet, levels, c.device, c.dtype).inverse(c)."""
    return Dwt(wavelet, levels, c.device, c.dtype).inverse(c)


def _host(fn, signal, wavelet, levels) -> np.ndarray:
    name, h, ntaps = _wavelet(wavelet)
    levels = integer(levels, "levels", 32)
    x, x2 = host_rows(signal)
    y = np.empty_like(x2)
    check(fn(_capi.dptr(x2), x2.shape[0], x2.shape[1], name, _capi.dptr(h), ntaps, levels, _capi.dptr(y)))
    return y.reshape(x.shape)


def wavedecHost(signal, wavelet, levels) -> np.ndarray:
    """Host f64 form (numpy in, numpy out) through pdsp_dwt_forward_host_f64: signal [n] or [..., n]."""
    return _host(lib.pdsp_dwt_forward_host_f64, signal, wavelet, levels)


def waverecHost(coeffs, wavelet, levels) -> np.ndarray:
    """Host f64 form (numpy in, numpy out) through pdsp_dwt_inverse_host_f64: coeffs [n] or [..., n]."""
    return _host(lib.pdsp_dwt_inverse_host_f64, coeffs, wavelet, levels)

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

from . import _capi
from ._capi import PdspError, check, lib
from .filters import _rows
from .resample import _host_rows

MAX_TAPS = 32


def _wavelet(wavelet):
    """(name bytes or None, taps array or None, ntaps) as the C ABI takes them."""
    if isinstance(wavelet, str):
        return wavelet.encode("utf-8"), None, 0
    if isinstance(wavelet, torch.Tensor):
        wavelet = wavelet.detach().cpu().numpy()
    h = np.ascontiguousarray(np.asarray(wavelet, dtype=np.float64).reshape(-1))
    return None, h, h.size


def _levels(levels) -> int:
    if isinstance(levels, bool) or not isinstance(levels, (int, np.integer)) or not -2 ** 31 <= int(levels) < 2 ** 31:
        raise PdspError(_capi.ERR_BAD_ARG, f"levels must be an integer, got {levels!r}")
    return int(levels)


def wavelet_taps(name: str) -> np.ndarray:
    """The scaling filter of a built-in wavelet: "haar" (= "db1"), "db2" ... "db10" (extremal phase, sum sqrt 2)."""
    if not isinstance(name, str):
        raise PdspError(_capi.ERR_BAD_ARG, f"wavelet name must be a string, got {name!r}")
    n = C.c_longlong()
    check(lib.pdsp_wavelet_taps(name.encode("utf-8"), None, C.byref(n)))
    h = np.empty(n.value, dtype=np.float64)
    check(lib.pdsp_wavelet_taps(name.encode("utf-8"), _capi.dptr(h), C.byref(n)))
    return h


class Dwt:
    """A pdsp_dwt on one GPU: `levels` levels of one orthogonal wavelet over rows along the last axis."""

    def __init__(self, wavelet, levels, device=None, dtype=torch.float32):
        if dtype not in (torch.float32, torch.float64):
            raise PdspError(_capi.ERR_BAD_ARG, f"unsupported dtype {dtype}")
        name, h, ntaps = _wavelet(wavelet)
        levels = _levels(levels)
        self.dtype = dtype
        self._sfx = "f32" if dtype == torch.float32 else "f64"
        self._h = C.c_void_p()
        if not torch.cuda.is_available():
            # argument errors come first, as everywhere: the library checks them without a device
            probe = C.c_void_p()
            check(lib.pdsp_dwt_create(-1, name, _capi.dptr(h), ntaps, levels, C.byref(probe)))
            lib.pdsp_dwt_destroy(probe)
            raise PdspError(_capi.ERR_DEVICE, "no HIP device available (the pdsp engine has no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        check(lib.pdsp_dwt_create(self.device.index, name, _capi.dptr(h), ntaps, levels, C.byref(self._h)))
        self.levels = int(lib.pdsp_dwt_levels(self._h))
        self.ntaps = int(lib.pdsp_dwt_ntaps(self._h))
        self.taps = np.empty(self.ntaps, dtype=np.float64)
        check(lib.pdsp_dwt_taps(self._h, _capi.dptr(self.taps)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib.pdsp_dwt_destroy(h)
            self._h = None

    def max_levels(self, length: int) -> int:
        """The deepest forward transform of rows of `length` values in this precision (0: none)."""
        return int(lib.pdsp_dwt_max_levels(self.ntaps, int(length), 4 if self.dtype == torch.float32 else 8))

    def _run(self, direction: str, x: torch.Tensor, out: torch.Tensor | None) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or x.dtype != self.dtype or not x.is_cuda or x.device != self.device:
            raise PdspError(_capi.ERR_BAD_ARG, f"input must be a {self.dtype} tensor on {self.device}")
        length = x.shape[-1] if x.dim() else 0
        rows, x_stride = _rows(x, "input")
        shape = tuple(x.shape)
        if out is None:
            out = torch.empty(shape, dtype=self.dtype, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.dtype != self.dtype or out.device != self.device
              or tuple(out.shape) != shape):
            raise PdspError(_capi.ERR_BAD_ARG, f"out must be a {self.dtype} tensor of shape {shape} on {self.device}")
        _, y_stride = _rows(out, "out")
        with torch.cuda.device(self.device):
            fn = getattr(lib, f"pdsp_dwt_{direction}_{self._sfx}")
            check(fn(self._h, rows, C.c_void_p(x.data_ptr()), length, x_stride, C.c_void_p(out.data_ptr()), y_stride,
                     C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return out

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
    levels = _levels(levels)
    x, x2 = _host_rows(signal)
    y = np.empty_like(x2)
    check(fn(_capi.dptr(x2), x2.shape[0], x2.shape[1], name, _capi.dptr(h), ntaps, levels, _capi.dptr(y)))
    return y.reshape(x.shape)


def wavedecHost(signal, wavelet, levels) -> np.ndarray:
    """Host f64 form (numpy in, numpy out) through pdsp_dwt_forward_host_f64: signal [n] or [..., n]."""
    return _host(lib.pdsp_dwt_forward_host_f64, signal, wavelet, levels)


def waverecHost(coeffs, wavelet, levels) -> np.ndarray:
    """Host f64 form (numpy in, numpy out) through pdsp_dwt_inverse_host_f64: coeffs [n] or [..., n]."""
    return _host(lib.pdsp_dwt_inverse_host_f64, coeffs, wavelet, levels)

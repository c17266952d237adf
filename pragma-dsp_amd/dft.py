"""The discrete Fourier transform of rows of ANY length, 2 <= L <= 4096 -- not only the powers of two of BatchedFft and
Radix2Fft -- by Bluestein's chirp-z algorithm, one launch per call (include/pdsp_hip.h, "any-length DFT").  The
conventions are numpy's fft / ifft along the last axis: X[k] = sum_n x[n] exp(-2 pi i n k / L), no scaling forward,
1 / L on the inverse.

    Dft(length, device=None)        the tables of one length on one GPU (f32 and f64)
      .forward(re, im=None, out=None) / .inverse(re, im, out=None)   torch planes [rows, L] -> (re, im)
    dft(x) / idft(X)                host f64 forms: numpy in (real or complex, [L] or [..., L]), complex128 out

A power-of-two length is accepted and takes the same kernel; BatchedFft is the fast way for those.  torch is used for
device memory and streams only; the arithmetic is the HIP kernel behind the C ABI.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _capi
from ._capi import PdspError, check, lib
from .filters import _rows

MIN_LENGTH = 2
MAX_LENGTH = 4096


def _length(length) -> int:
    if isinstance(length, bool) or not isinstance(length, (int, np.integer)) or not -2 ** 63 <= int(length) < 2 ** 63:
        raise PdspError(_capi.ERR_BAD_ARG, f"length must be an integer, got {length!r}")
    return int(length)


class Dft:
    """A pdsp_dft on one GPU: the chirp and chirp-filter tables of one length, both precisions."""

    def __init__(self, length, device=None):
        length = _length(length)
        self._h = C.c_void_p()
        if not torch.cuda.is_available():
            # argument errors come first, as everywhere: the library checks them without a device
            check(lib.pdsp_dft_create(length, -1, C.byref(self._h)))
            raise PdspError(_capi.ERR_DEVICE, "no HIP device available (the pdsp engine has no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        check(lib.pdsp_dft_create(length, self.device.index, C.byref(self._h)))
        self.length = int(lib.pdsp_dft_length(self._h))
        self.conv_size = int(lib.pdsp_dft_conv_size(self._h))  # M, the points of the circular convolution

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib.pdsp_dft_destroy(h)
            self._h = None

    def _plane(self, t, name, like=None):
        if (not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.float64) or not t.is_cuda
                or t.device != self.device or t.dim() == 0 or t.shape[-1] != self.length):
            raise PdspError(_capi.ERR_BAD_ARG,
                            f"{name} must be a float32 or float64 tensor [..., {self.length}] on {self.device}")
        if like is not None and (t.dtype != like.dtype or t.shape != like.shape):
            raise PdspError(_capi.ERR_BAD_ARG, f"{name} must have the dtype and shape of re")
        return _rows(t, name)

    def _run(self, re, im, out, inverse):
        rows, stride = self._plane(re, "re")
        if im is not None and self._plane(im, "im", re) != (rows, stride):
            raise PdspError(_capi.ERR_BAD_ARG, "re and im must have the same row stride")
        if out is None:
            out = (torch.empty(re.shape, dtype=re.dtype, device=self.device),
                   torch.empty(re.shape, dtype=re.dtype, device=self.device))
        elif not isinstance(out, (tuple, list)) or len(out) != 2:
            raise PdspError(_capi.ERR_BAD_ARG, "out must be a pair of tensors (re, im)")
        o_rows = [self._plane(o, "out", re) for o in out]
        if o_rows[0] != o_rows[1]:
            raise PdspError(_capi.ERR_BAD_ARG, "the two out planes must have the same row stride")
        with torch.cuda.device(self.device):
            fn = lib.pdsp_dft_c2c_f32 if re.dtype == torch.float32 else lib.pdsp_dft_c2c_f64
            check(fn(self._h, rows, C.c_void_p(re.data_ptr()), C.c_void_p(im.data_ptr()) if im is not None else None,
                     stride, C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()), o_rows[0][1], int(inverse),
                     C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return out[0], out[1]

    def forward(self, re: torch.Tensor, im: torch.Tensor | None = None, out=None):
        """Rows along the last axis ([..., L] contiguous, or a 2-D view with a row stride >= L) -> (re, im); im None
        means real rows.  One launch on the current stream."""
        return self._run(re, im, out, False)

    def inverse(self, re: torch.Tensor, im: torch.Tensor, out=None):
        """The inverse transform of the rows (re, im), scaled by 1 / L -> (re, im)."""
        if im is None:
            raise PdspError(_capi.ERR_BAD_ARG, "the inverse needs both planes")
        return self._run(re, im, out, True)


def _host(x, inverse: bool) -> np.ndarray:
    a = np.asarray(x)
    cplx = np.iscomplexobj(a)
    a = np.asarray(a, dtype=np.complex128 if cplx else np.float64)
    if a.ndim == 0:
        raise PdspError(_capi.ERR_BAD_ARG, "x must have at least one axis")
    ln = a.shape[-1]
    rows = int(np.prod(a.shape[:-1], dtype=np.int64))
    re = np.ascontiguousarray(a.real).reshape(rows, ln)
    im = np.ascontiguousarray(a.imag).reshape(rows, ln) if cplx else None
    # a length the library refuses gets no buffers: the library fails before it writes
    n = ln if MIN_LENGTH <= ln <= MAX_LENGTH else 0
    ore, oim = np.empty((rows, n), dtype=np.float64), np.empty((rows, n), dtype=np.float64)
    check(lib.pdsp_dft_host_f64(_capi.dptr(re), _capi.dptr(im), rows, ln, int(inverse), _capi.dptr(ore),
                                _capi.dptr(oim)))
    return (ore + 1j * oim).reshape(a.shape)


def dft(x) -> np.ndarray:
    """The DFT of x along its last axis (any length 2 ... 4096), computed on the device in f64: complex128."""
    return _host(x, False)


def idft(x) -> np.ndarray:
    """The inverse DFT of x along its last axis, scaled by 1 / L, computed on the device in f64: complex128."""
    return _host(x, True)

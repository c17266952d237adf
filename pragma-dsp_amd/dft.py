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

import numpy as np
import torch

from . import _capi
from ._capi import PdspError, lib
from ._chirp import ChirpRows, host_call, host_planes, integer

MIN_LENGTH = 2
MAX_LENGTH = 4096


class Dft(ChirpRows):
    """A pdsp_dft on one GPU: the chirp and chirp-filter tables of one length, both precisions."""

    _destroy = lib.pdsp_dft_destroy

    def _entry(self, sfx):
        return getattr(lib, "pdsp_dft_c2c_" + sfx)

    def __init__(self, length, device=None):
        self._create(lib.pdsp_dft_create, device, integer(length, "length"))
        self.length = self.bins = int(lib.pdsp_dft_length(self._h))
        self.conv_size = int(lib.pdsp_dft_conv_size(self._h))  # M, the points of the circular convolution

    def forward(self, re: torch.Tensor, im: torch.Tensor | None = None, out=None):
        """Rows along the last axis ([..., L] contiguous, or a 2-D view with a row stride >= L) -> (re, im); im None
        means real rows.  One launch on the current stream."""
        return self._run(re, im, out, 0)

    def inverse(self, re: torch.Tensor, im: torch.Tensor, out=None):
        """The inverse transform of the rows (re, im), scaled by 1 / L -> (re, im)."""
        if im is None:
            raise PdspError(_capi.ERR_BAD_ARG, "the inverse needs both planes")
        return self._run(re, im, out, 1)


def _host(x, inverse: bool) -> np.ndarray:
    a, re, im = host_planes(x)
    ln = a.shape[-1]
    return host_call(lib.pdsp_dft_host_f64, a, re, im, ln, MIN_LENGTH <= ln <= MAX_LENGTH, int(inverse))


def dft(x) -> np.ndarray:
    """The DFT of x along its last axis (any length 2 ... 4096), computed on the device in f64: complex128."""
    return _host(x, False)


def idft(x) -> np.ndarray:
    """The inverse DFT of x along its last axis, scaled by 1 / L, computed on the device in f64: complex128."""
    return _host(x, True)

"""The transform over the last two axes of batched images, numpy's fft2 / ifft2 (include/pdsp_hip_fft2d.h):
X[k][l] = sum_h sum_w x[h][w] exp(-2 pi i (h k / H + w l / W)), planar complex, f32 and f64, H and W powers of two with
16 <= H <= 512 and 16 <= W <= 16384 (f64: 8192).  Images of up to 4096 points are transformed in one launch and one
pass over memory by workgroups that hold whole images in LDS; larger ones take the 1-D row kernels and one column
launch.  No scratch, no torch transposes.

    Fft2d(height, width, device=None)     the object of one image shape on one GPU (f32 and f64)
      .forward(re, im=None, out=None, norm=None) / .inverse(re, im, out=None, norm=None)
                                          torch planes [..., H, W] -> (re, im), on the current stream
      .path                               "resident" or "two-pass" (per precision: .query(dtype))
    fft2(x, norm=None) / ifft2(x, norm=None)   host f64 forms: numpy in (real or complex, [..., H, W]), complex128 out

norm is numpy's: None / "backward", "ortho", "forward".  torch is used for device memory and streams only; the
arithmetic is the HIP kernels behind the C ABI.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from . import _capi, _device
from ._capi import PdspError, check, lib
from ._device import integer, operand, ptr

NORMS = {None: 0, "backward": 0, "ortho": 1, "forward": 2}
PATHS = ("resident", "two-pass")
QUERY_FIELDS = ("path", "images_per_workgroup", "tile", "launches")


def _norm(norm) -> int:
    if norm not in NORMS:
        raise PdspError(_capi.ERR_BAD_ARG, f'norm must be None, "backward", "ortho" or "forward", got {norm!r}')
    return NORMS[norm]


def query(height, width, dtype=torch.float32) -> dict:
    """pdsp_fft2d_query by field name: the path a shape takes in a precision, images per workgroup (resident), the
    column tile (two-pass) and the launches per call.  Host only; raises outside the domain."""
    info = (C.c_int * len(QUERY_FIELDS))()
    elem = 4 if _device.suffix(dtype) == "f32" else 8
    check(lib.pdsp_fft2d_query(integer(height, "height"), integer(width, "width"), elem, info))
    d = dict(zip(QUERY_FIELDS, info))
    d["path"] = PATHS[d["path"]]
    return d


class Fft2d(_device.Handle):
    """A pdsp_fft2d on one GPU: the plans of W and H points, both precisions, every table uploaded here."""

    _destroy = lib.pdsp_fft2d_destroy

    def __init__(self, height, width, device=None):
        h, w = integer(height, "height"), integer(width, "width")
        self._open(lambda dev, out: lib.pdsp_fft2d_create(h, w, dev, out), device)
        self.height = int(lib.pdsp_fft2d_height(self._h))
        self.width = int(lib.pdsp_fft2d_width(self._h))
        self.path = self.query(torch.float32)["path"]

    def query(self, dtype=torch.float32) -> dict:
        return query(self.height, self.width, dtype)

    def _run(self, re, im, out, inverse, norm):
        code = _norm(norm)
        operand(re, "re", self.device)
        if re.dtype not in _device.SFX or re.dim() < 2 or tuple(re.shape[-2:]) != (self.height, self.width):
            raise PdspError(_capi.ERR_BAD_ARG, f"re must be a float32 or float64 tensor [..., {self.height}, "
                                               f"{self.width}] on {self.device}")
        if im is not None:
            operand(im, "im", self.device, re.dtype, shape=re.shape)
        if out is None:
            out = (torch.empty_like(re), torch.empty_like(re))
        elif not isinstance(out, (tuple, list)) or len(out) != 2:
            raise PdspError(_capi.ERR_BAD_ARG, "out must be a pair of tensors (re, im)")
        for o in out:
            operand(o, "out", self.device, re.dtype, shape=re.shape)
        batch = math.prod(re.shape[:-2])
        if batch == 0:
            return out[0], out[1]
        with torch.cuda.device(self.device):
            fn = getattr(lib, "pdsp_fft2d_c2c_" + _device.SFX[re.dtype])
            check(fn(self._h, batch, ptr(re), ptr(im) if im is not None else None, ptr(out[0]), ptr(out[1]),
                     int(inverse), code, _device.stream_ptr(self.device)))
        return out[0], out[1]

    def forward(self, re: torch.Tensor, im: torch.Tensor | None = None, out=None, norm=None):
        """Images over the last two axes ([..., H, W] contiguous) -> (re, im); im None means real images.  out may be
        the inputs themselves (in place), and nothing else that overlaps them."""
        return self._run(re, im, out, 0, norm)

    def inverse(self, re: torch.Tensor, im: torch.Tensor, out=None, norm=None):
        """The inverse transform of the images (re, im), scaled by 1 / (H W) unless norm says otherwise -> (re, im)."""
        if im is None:
            raise PdspError(_capi.ERR_BAD_ARG, "the inverse needs both planes")
        return self._run(re, im, out, 1, norm)


def _host(x, inverse: bool, norm) -> np.ndarray:
    code = _norm(norm)
    a = np.asarray(x)
    cplx = np.iscomplexobj(a)
    a = np.asarray(a, dtype=np.complex128 if cplx else np.float64)
    if a.ndim < 2:
        raise PdspError(_capi.ERR_BAD_ARG, "x must have at least two axes [..., H, W]")
    h, w = a.shape[-2:]
    batch = math.prod(a.shape[:-2])
    re = np.ascontiguousarray(a.real, dtype=np.float64)
    im = np.ascontiguousarray(a.imag, dtype=np.float64) if cplx else None
    if inverse and im is None:
        im = np.zeros_like(re)
    ore, oim = np.empty_like(re), np.empty_like(re)
    check(lib.pdsp_fft2d_host_f64(_capi.dptr(re), _capi.dptr(im), batch, h, w, int(inverse), code, _capi.dptr(ore),
                                  _capi.dptr(oim)))
    return ore + 1j * oim


def fft2(x, norm=None) -> np.ndarray:
    """numpy's fft2 of x over its last two axes, computed on the device in f64: complex128."""
    return _host(x, False, norm)


def ifft2(x, norm=None) -> np.ndarray:
    """numpy's ifft2 of x over its last two axes, computed on the device in f64: complex128."""
    return _host(x, True, norm)

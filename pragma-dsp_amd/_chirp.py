"""What Dft and Czt share.  Both are handles of the library's chirp-z rows (the DFT is the chirp-z transform with as
many bins as samples, on the whole circle), so the integer check, the handle's life and device, the validation of the
planes and of the out pair, the ctypes call and the two halves of the host forms are written once.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _capi
from ._capi import PdspError, check
from .filters import _rows


def integer(v, name) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -2 ** 63 <= int(v) < 2 ** 63:
        raise PdspError(_capi.ERR_BAD_ARG, f"{name} must be an integer, got {v!r}")
    return int(v)


class ChirpRows:
    """A handle of the library on one GPU that takes rows [..., length] to rows [..., bins]; the subclass names the
    library's functions and sets length and bins."""

    _destroy = None  # the library's destroy function
    _forward = None  # its (f32, f64) entry points

    def _create(self, create, device, *args):
        """self._h = create(*args, device index, &handle), and self.device."""
        self._h = C.c_void_p()
        if not torch.cuda.is_available():
            # argument errors come first, as everywhere: the library checks them without a device
            check(create(*args, -1, C.byref(self._h)))
            raise PdspError(_capi.ERR_DEVICE, "no HIP device available (the pdsp engine has no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        check(create(*args, self.device.index, C.byref(self._h)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            type(self)._destroy(h)
            self._h = None

    def _plane(self, t, name, width, like=None, shape=None):
        if (not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.float64) or not t.is_cuda
                or t.device != self.device or t.dim() == 0 or t.shape[-1] != width):
            raise PdspError(_capi.ERR_BAD_ARG,
                            f"{name} must be a float32 or float64 tensor [..., {width}] on {self.device}")
        if like is not None and (t.dtype != like.dtype or tuple(t.shape) != tuple(shape)):
            raise PdspError(_capi.ERR_BAD_ARG, f"{name} must have the dtype of re and the shape {tuple(shape)}")
        return _rows(t, name)

    def _run(self, re, im, out, *tail):
        """One launch on the current stream; tail: the entry point's arguments between out_stride and the stream."""
        rows, stride = self._plane(re, "re", self.length)
        if im is not None and self._plane(im, "im", self.length, re, re.shape) != (rows, stride):
            raise PdspError(_capi.ERR_BAD_ARG, "re and im must have the same row stride")
        oshape = tuple(re.shape[:-1]) + (self.bins,)
        if out is None:
            out = (torch.empty(oshape, dtype=re.dtype, device=self.device),
                   torch.empty(oshape, dtype=re.dtype, device=self.device))
        elif not isinstance(out, (tuple, list)) or len(out) != 2:
            raise PdspError(_capi.ERR_BAD_ARG, "out must be a pair of tensors (re, im)")
        o_rows = [self._plane(o, "out", self.bins, re, oshape) for o in out]
        if o_rows[0] != o_rows[1]:
            raise PdspError(_capi.ERR_BAD_ARG, "the two out planes must have the same row stride")
        with torch.cuda.device(self.device):
            fn = type(self)._forward[re.dtype == torch.float64]
            check(fn(self._h, rows, C.c_void_p(re.data_ptr()), C.c_void_p(im.data_ptr()) if im is not None else None,
                     stride, C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()), o_rows[0][1], *tail,
                     C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return out[0], out[1]


def host_planes(x):
    """numpy in (real or complex, [L] or [..., L]) -> (the array, re [rows, L], im [rows, L] or None)."""
    a = np.asarray(x)
    cplx = np.iscomplexobj(a)
    a = np.asarray(a, dtype=np.complex128 if cplx else np.float64)
    if a.ndim == 0:
        raise PdspError(_capi.ERR_BAD_ARG, "x must have at least one axis")
    rows = int(np.prod(a.shape[:-1], dtype=np.int64))
    re = np.ascontiguousarray(a.real).reshape(rows, a.shape[-1])
    im = np.ascontiguousarray(a.imag).reshape(rows, a.shape[-1]) if cplx else None
    return a, re, im


def host_call(fn, a, re, im, bins, accepted, *mid):
    """fn(re, im, rows, L, *mid, out re, out im) -> complex128 [..., bins].  Sizes the library refuses (accepted false)
    get no buffers: the library fails before it writes."""
    rows, ln = re.shape
    ore, oim = (np.empty((rows, bins if accepted else 0), dtype=np.float64) for _ in range(2))
    check(fn(_capi.dptr(re), _capi.dptr(im), rows, ln, *mid, _capi.dptr(ore), _capi.dptr(oim)))
    return (ore + 1j * oim).reshape(a.shape[:-1] + (bins,))

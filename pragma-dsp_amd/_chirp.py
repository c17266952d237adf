"""What Dft and Czt share.  Both are handles of the library's chirp-z rows (the DFT is the chirp-z transform with as
many bins as samples, on the whole circle), so the validation of the planes and of the out pair, the ctypes call and
the two halves of the host forms are written once; the handle's life and the operand checks are _device.py's.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _capi, _device
from ._capi import PdspError, check
from ._device import integer, operand, ptr, rows  # noqa: F401  (integer: for dft.py and czt.py)


class ChirpRows(_device.Handle):
    """A handle of the library on one GPU that takes rows [..., length] to rows [..., bins]; the subclass names the
    library's functions and sets length and bins."""

    def _entry(self, sfx):
        """The forward entry point of a precision, looked up through the subclass's module."""
        raise NotImplementedError

    def _create(self, create, device, *args):
        """self._h = create(*args, device index, &handle), and self.device."""
        self._open(lambda dev, out: create(*args, dev, out), device)

    # Not _device.launch_rows: two planes in and two out, of either precision, with an optional im and a pairwise
    # stride rule.
    def _run(self, re, im, out, *tail):
        """One launch on the current stream; tail: the entry point's arguments between out_stride and the stream."""
        operand(re, "re", self.device, layout="rows")
        if re.dtype not in _device.SFX or re.dim() == 0 or re.shape[-1] != self.length:
            raise PdspError(_capi.ERR_BAD_ARG,
                            f"re must be a float32 or float64 tensor [..., {self.length}] on {self.device}")
        n, stride = rows(re, "re")
        if im is not None:
            operand(im, "im", self.device, re.dtype, shape=re.shape, layout="rows")
            if rows(im, "im")[1] != stride:
                raise PdspError(_capi.ERR_BAD_ARG, "re and im must have the same row stride")
        oshape = re.shape[:-1] + (self.bins,)
        if out is None:
            out = (torch.empty(oshape, dtype=re.dtype, device=self.device),
                   torch.empty(oshape, dtype=re.dtype, device=self.device))
        elif not isinstance(out, (tuple, list)) or len(out) != 2:
            raise PdspError(_capi.ERR_BAD_ARG, "out must be a pair of tensors (re, im)")
        for o in out:
            operand(o, "out", self.device, re.dtype, shape=oshape, layout="rows")
        o_stride = rows(out[0], "out")[1]
        if rows(out[1], "out")[1] != o_stride:
            raise PdspError(_capi.ERR_BAD_ARG, "the two out planes must have the same row stride")
        with torch.cuda.device(self.device):
            fn = self._entry(_device.SFX[re.dtype])
            check(fn(self._h, n, ptr(re), ptr(im) if im is not None else None, stride, ptr(out[0]), ptr(out[1]),
                     o_stride, *tail, _device.stream_ptr(self.device)))
        return out[0], out[1]


def host_planes(x):
    """numpy in (real or complex, [L] or [..., L]) -> (the array, re [rows, L], im [rows, L] or None)."""
    a = np.asarray(x)
    cplx = np.iscomplexobj(a)
    a = np.asarray(a, dtype=np.complex128 if cplx else np.float64)
    re = _device.host_rows(a.real, "x")[1]
    im = _device.host_rows(a.imag, "x")[1] if cplx else None
    return a, re, im


def host_call(fn, a, re, im, bins, accepted, *mid):
    """fn(re, im, rows, L, *mid, out re, out im) -> complex128 [..., bins].  Sizes the library refuses (accepted false)
    get no buffers: the library fails before it writes."""
    rows, ln = re.shape
    ore, oim = (np.empty((rows, bins if accepted else 0), dtype=np.float64) for _ in range(2))
    check(fn(_capi.dptr(re), _capi.dptr(im), rows, ln, *mid, _capi.dptr(ore), _capi.dptr(oim)))
    return (ore + 1j * oim).reshape(a.shape[:-1] + (bins,))

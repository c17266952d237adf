"""What every device entry point of the Python layer shares.  The library takes raw device pointers and cannot know
how many bytes lie behind one, so every bounds guarantee of the device API rests on the checks made here: the operand
validator, the rows rule, the integer check, device resolution, the handle base and the rows-in / rows-out launch.

Helpers validate, modules call: nothing in this file looks an entry point up.  Each module resolves its functions
through its own module-level `lib` (which tests replace by stand-ins) and hands them in.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import torch

from ._capi import ERR_BAD_ARG, ERR_DEVICE, ERR_INPUT_LENGTH, PdspError, check

SFX = {torch.float32: "f32", torch.float64: "f64"}
COMPLEX = {torch.float32: torch.complex64, torch.float64: torch.complex128}


def stream_ptr(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device.index).cuda_stream)  # by index: torch's short path


def ptr(t) -> C.c_void_p:
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def suffix(dtype, what=None) -> str:
    """"f32" / "f64", the ending of the entry points of a precision."""
    sfx = SFX.get(dtype)
    if sfx is None:
        raise PdspError(ERR_BAD_ARG, (f"{what}: " if what else "") + f"unsupported dtype {dtype} (float32 or float64)")
    return sfx


def resolve_device(device) -> torch.device:
    """The indexed CUDA device a handle lives on; None and "cuda" mean the current one."""
    if not torch.cuda.is_available():
        raise PdspError(ERR_DEVICE, "no HIP device available (the pdsp engine has no CPU fallback)")
    dev = torch.device("cuda") if device is None else torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def integer(v, name, bits=64) -> int:
    lim = 1 << (bits - 1)
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -lim <= int(v) < lim:
        raise PdspError(ERR_BAD_ARG, f"{name} must be an integer, got {v!r}")
    return int(v)


def rows(t: torch.Tensor, name: str):
    """(rows, row stride) of a tensor of rows [..., len]: contiguous, or 2-D with unit stride along the row."""
    if t.dim() == 0:
        raise PdspError(ERR_BAD_ARG, f"{name} must have at least one axis")
    if t.is_contiguous():
        return math.prod(t.shape[:-1]), t.shape[-1]
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
        return t.shape[0], t.stride(0)
    raise PdspError(ERR_BAD_ARG, f"{name}: rows at a stride are taken in 2-D tensors only")


def operand(t, name, device=None, dtype=None, *, ndim=None, shape=None, last=None, numel=None, layout="contiguous"):
    """One tensor the library will read or write through a raw pointer: a CUDA tensor, on `device` (a CUDA device)
    and of `dtype` where given, with `ndim` axes, exactly `shape`, a last axis of `last` values, `numel` elements; laid out
    "contiguous", as 2-D "strided" rows (unit stride along the row, any row stride >= the row), or as "rows" (what
    rows() takes, which the caller asks next)."""
    if not isinstance(t, torch.Tensor) or (not t.is_cuda if device is None else t.device != device) \
            or (dtype is not None and t.dtype != dtype):
        raise PdspError(ERR_BAD_ARG, f"{name} must be a {'' if dtype is None else str(dtype) + ' '}tensor on "
                                     f"{'a CUDA device' if device is None else device}")
    if ndim is not None and t.dim() != ndim:
        raise PdspError(ERR_BAD_ARG, f"{name} must be a {ndim}-D tensor")
    if shape is not None and t.shape != shape:
        raise PdspError(ERR_BAD_ARG, f"{name} must be a tensor of shape {tuple(shape)}, got {tuple(t.shape)}")
    if last is not None and t.shape[-1] != last:
        raise PdspError(ERR_INPUT_LENGTH, f"FFT input length {t.shape[-1]} != size {last}")
    if numel is not None and t.numel() != numel:
        raise PdspError(ERR_INPUT_LENGTH, f"{name} has {t.numel()} elements, {numel} expected")
    if layout == "contiguous":
        if not t.is_contiguous():
            raise PdspError(ERR_BAD_ARG, f"{name} must be contiguous")
    elif layout == "strided" and (t.shape[0] > 1 and t.stride(0) < t.shape[1] or (t.shape[1] > 1 and t.stride(1) != 1)):
        raise PdspError(ERR_BAD_ARG, f"{name} needs contiguous rows at a row stride >= the row")


def host_rows(x, name="signal"):
    """numpy in ([len] or [..., len]) -> (the array as contiguous f64, its rows [rows, len])."""
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    if a.ndim == 0:
        raise PdspError(ERR_BAD_ARG, f"{name} must have at least one axis")
    return a, a.reshape(math.prod(a.shape[:-1]), a.shape[-1])


class Handle:
    """A handle of the library on one GPU: `device`, `_h`, and for the classes of one precision `dtype` / `_sfx`.  The
    subclass names the library's destroy function."""

    _destroy = None
    _h = None

    def _open(self, create, device, dtype=None):
        """self._h = create(device index, &handle), and self.device.  Argument errors come first, as everywhere: the
        library checks them without a device."""
        if dtype is not None:
            self.dtype, self._sfx = dtype, suffix(dtype)
        self._h = C.c_void_p()
        if not torch.cuda.is_available():
            check(create(-1, C.byref(self._h)))
            self.close()
        self.device = resolve_device(device)
        check(create(self.device.index, C.byref(self._h)))

    def close(self):
        """Destroys the native handle now (also done when the object is collected)."""
        h, self._h = self._h, None
        if h:
            self._destroy(h)

    def __del__(self):
        self.close()


def launch_rows(fn, h, owner, x, out, y_len, before=(), between=()):
    """The rows-in / rows-out launch on the current stream: fn(h, rows, x, len, x_stride, *before, out, *between,
    out_stride, stream) with x [..., len] -- which the caller, who needed len for y_len, has put through operand(x,
    "input", device, dtype, layout="rows") -- and out [..., y_len], allocated here, or the caller's, of exactly that
    shape; each contiguous or a 2-D view with a row stride, on owner.device and of owner.dtype."""
    device, dtype = owner.device, owner.dtype
    n, x_stride = rows(x, "input")
    shape = (*x.shape[:-1], y_len)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=device)
    else:
        operand(out, "out", device, dtype, shape=shape, layout="rows")
    _, y_stride = rows(out, "out")
    with torch.cuda.device(device):
        check(fn(h, n, ptr(x), x.shape[-1], x_stride, *before, ptr(out), *between, y_stride, stream_ptr(device)))
    return out

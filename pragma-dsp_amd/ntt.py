"""The number-theoretic transform over GF(p), p = 2^64 - 2^32 + 1, and exact integer convolution on the device
(include/pdsp_hip.h, "number-theoretic transform").  The reference's roadmap lists it as section F ("NTT / finite-field
transforms: field abstractions, NTT forward/inverse, polynomial multiplication utilities") and has no such code yet, so
the definition is this library's own:

    X[k] = sum_n x[n] w^(n k) mod p          x[n] = N^-1 sum_k X[k] w^(-n k) mod p          w = 7^((p - 1) / N) mod p

natural order in and out, N = 2^k, 64 <= N <= 16384.  An element is 64 bits: any pattern goes in (taken mod p), a
canonical value in [0, p) comes out.  Nothing is rounded, so every path gives the same bits.

    Ntt(size, device=None)     .forward(x) / .inverse(X) / .convolve(a, b, out_len=None)      device rows
    ntt_mul(a, b)                                                       element-wise a b mod p on the device
    ntt(x) / intt(x) / polymul(a, b)                                    host forms, numpy uint64 in and out
    convolve_exact(a, b)                                                exact linear convolution of signed integers
    NTT_MODULUS, ntt_root(n)                                            p and w as Python integers

Device tensors are torch.uint64 or torch.int64 (the same bits); the output has the input's dtype.  torch is used for
device memory and streams only; the arithmetic is the HIP kernel behind the C ABI.
"""
from __future__ import annotations

import ctypes as C
import math
from types import SimpleNamespace

import numpy as np
import torch

from . import _capi, _device
from ._capi import ERR_BAD_ARG, PdspError, check, lib
from ._device import integer

NTT_MODULUS = int(lib.pdsp_ntt_modulus())
MIN_SIZE, MAX_SIZE = 64, 16384
_DTYPES = (torch.uint64, torch.int64)


def ntt_root(n: int) -> int:
    """w_n = 7^((p - 1) / n) mod p, n a power of two up to 2^32."""
    n = integer(n, "n")
    w = int(lib.pdsp_ntt_root(n))
    if w == 0:
        raise PdspError(ERR_BAD_ARG, f"n must be a power of two, 1 ... 2^32, got {n}")
    return w


def _words(t, name, device=None):
    """A device tensor of 64-bit words: uint64 or int64."""
    if not isinstance(t, torch.Tensor) or t.dtype not in _DTYPES:
        raise PdspError(ERR_BAD_ARG, f"{name} must be a torch.uint64 or torch.int64 tensor on "
                                     f"{'a CUDA device' if device is None else device}")
    return t.dtype


class Ntt(_device.Handle):
    """A pdsp_ntt on one GPU: transforms and cyclic convolutions of rows of `size` points along the last axis."""

    _destroy = lib.pdsp_ntt_destroy

    def __init__(self, size, device=None):
        size = integer(size, "size")
        self._open(lambda dev, out: lib.pdsp_ntt_create(size, dev, out), device)
        self.size = int(lib.pdsp_ntt_size(self._h))

    def _run(self, fn, x, out):
        dtype = _words(x, "input", self.device)
        _device.operand(x, "input", self.device, dtype, last=self.size, layout="rows")
        return _device.launch_rows(lambda h, n, px, _len, xs, po, ys, st: fn(h, n, px, xs, po, ys, st), self._h,
                                   SimpleNamespace(device=self.device, dtype=dtype), x, out, self.size)

    def forward(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """Rows of `size` values ([..., size], contiguous or a 2-D view with a row stride) -> rows of their transform.
        out may be x itself."""
        return self._run(lib.pdsp_ntt_forward_u64, x, out)

    def inverse(self, X: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """Rows of transform values -> rows of points: inverse(forward(x)) == x mod p."""
        return self._run(lib.pdsp_ntt_inverse_u64, X, out)

    __call__ = forward

    def convolve(self, a: torch.Tensor, b: torch.Tensor, out_len=None, out: torch.Tensor | None = None) -> torch.Tensor:
        """c[i] = sum_{j + l = i mod size} a[j] b[l] mod p, i < out_len, in one launch.  a [..., a_len] and b
        ([..., b_len] with a's rows, or one row shared by all of them), both zero-padded to `size`; out_len defaults to
        min(a_len + b_len - 1, size): the linear product where it fits.  out may be a itself."""
        dtype = _words(a, "input", self.device)
        _device.operand(a, "input", self.device, dtype, layout="rows")
        _device.operand(b, "b", self.device, dtype, layout="rows")
        a_len, b_len = a.shape[-1], b.shape[-1]
        out_len = min(a_len + b_len - 1, self.size) if out_len is None else integer(out_len, "out_len")
        a_rows, _ = _device.rows(a, "input")
        b_rows, b_stride = _device.rows(b, "b")
        if b_rows == 1 and (b.dim() == 1 or a_rows != 1):
            b_stride = 0
        elif b_rows != a_rows:
            raise PdspError(ERR_BAD_ARG, f"b must have the input's {a_rows} rows or one row, got {b_rows}")
        return _device.launch_rows(lib.pdsp_ntt_conv_u64, self._h, SimpleNamespace(device=self.device, dtype=dtype), a,
                                   out, out_len, before=(_device.ptr(b), b_len, b_stride), between=(out_len,))


def ntt_mul(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """out = a b mod p, element by element: tensors of one shape, dtype (uint64 or int64) and device.  out may be a or
    b itself."""
    dtype = _words(a, "a")
    _device.operand(a, "a", None, dtype)
    _device.operand(b, "b", a.device, dtype, shape=a.shape)
    if out is None:
        out = torch.empty_like(a)
    else:
        _device.operand(out, "out", a.device, dtype, shape=a.shape)
    with torch.cuda.device(a.device):
        check(lib.pdsp_ntt_mul_u64(a.numel(), _device.ptr(a), _device.ptr(b), _device.ptr(out),
                                   _device.stream_ptr(a.device)))
    return out


# ---- host forms ------------------------------------------------------------------------------------------------------


def _host_words(x, name):
    """numpy in ([len] or [..., len], uint64 or int64) -> (the array as contiguous uint64, its rows [rows, len])."""
    a = np.asarray(x)
    if a.dtype not in (np.uint64, np.int64):
        raise PdspError(ERR_BAD_ARG, f"{name} must be an array of uint64 or int64, got {a.dtype}")
    if a.ndim == 0:
        raise PdspError(ERR_BAD_ARG, f"{name} must have at least one axis")
    a = np.ascontiguousarray(a).view(np.uint64)
    return a, a.reshape(math.prod(a.shape[:-1]), a.shape[-1])


def _vptr(a):
    return C.c_void_p(a.ctypes.data)


def _transform(x, inverse):
    a, a2 = _host_words(x, "input")
    y = np.empty_like(a2)
    check(lib.pdsp_ntt_host_u64(_vptr(a2), a2.shape[0], a2.shape[1], inverse, _vptr(y)))
    return y.reshape(a.shape)


def ntt(x) -> np.ndarray:
    """Host form (numpy in, numpy uint64 out) through pdsp_ntt_host_u64: x [n] or [..., n], n the transform size."""
    return _transform(x, 0)


def intt(x) -> np.ndarray:
    """Host form of the inverse transform."""
    return _transform(x, 1)


def _linear_size(a_len, b_len):
    n = max(MIN_SIZE, 1 << max(a_len + b_len - 2, 0).bit_length())
    if a_len < 1 or b_len < 1 or n > MAX_SIZE:
        raise PdspError(_capi.ERR_UNSUPPORTED_SIZE if n > MAX_SIZE else ERR_BAD_ARG,
                        f"the product of rows of {a_len} and {b_len} values needs a transform of 1 ... {MAX_SIZE} points")
    return n


def polymul(a, b) -> np.ndarray:
    """The linear product mod p of rows of coefficients: a [..., la], b [lb] or [..., lb] with a's rows -> [..., la + lb
    - 1], on the transform of the next power of two >= la + lb - 1, at least 64."""
    a, a2 = _host_words(a, "a")
    b, b2 = _host_words(b, "b")
    if b2.shape[0] != a2.shape[0] and b.ndim != 1:
        raise PdspError(ERR_BAD_ARG, f"b must have a's {a2.shape[0]} rows or be one row, got {b2.shape[0]}")
    la, lb = a2.shape[1], b2.shape[1]
    n = _linear_size(la, lb)
    y = np.empty((a2.shape[0], la + lb - 1), dtype=np.uint64)
    check(lib.pdsp_ntt_conv_host_u64(_vptr(a2), la, _vptr(b2), lb, int(b.ndim == 1), a2.shape[0], n, _vptr(y),
                                     la + lb - 1))
    return y.reshape(*a.shape[:-1], la + lb - 1)


def convolve_exact(a, b) -> np.ndarray:
    """The exact linear convolution of rows of signed integers, int64 out: a [..., la], b [lb] or [..., lb].  Negative
    values go in as p - |x| and residues above p / 2 come out negative; refused unless min(la, lb) max|a| max|b| <
    2^62, the bound below which every result is exact and fits."""
    a, b = np.asarray(a), np.asarray(b)
    for v, name in ((a, "a"), (b, "b")):
        if v.dtype.kind not in "iu" or v.ndim == 0:
            raise PdspError(ERR_BAD_ARG, f"{name} must be an array of integers with at least one axis, got {v.dtype}")
    la, lb = a.shape[-1], b.shape[-1]
    peak = [max((abs(int(v.min())), abs(int(v.max()))), default=0) if v.size else 0 for v in (a, b)]
    if min(la, lb) * peak[0] * peak[1] >= 1 << 62:
        raise PdspError(ERR_BAD_ARG, f"min(len a, len b) max|a| max|b| = {min(la, lb)} x {peak[0]} x {peak[1]} must be "
                                     "below 2^62 for an exact int64 result")
    p = np.uint64(NTT_MODULUS)

    def residues(v):  # x >= 0: x; x < 0: p - |x| = p + x in wrapping 64-bit arithmetic
        w = v.astype(np.int64).view(np.uint64)
        return np.where(v < 0, w + p, w)

    c = polymul(residues(a), residues(b))
    return np.where(c > p // np.uint64(2), c - p, c).view(np.int64)

"""The NTT's device-free half: the reference helper pinned to the definition, the field helpers of the C ABI (which
call the header the kernels compute with) against Python integers, every refusal of the C ABI with its code and exact
text, the Python layer's operand checks against a stand-in library, and convolve_exact's bound.  Every library call
here ends in a refusal, needs no device, or (without one) stops at PDSP_ERR_DEVICE after its argument checks."""
import ctypes as C
import random

import numpy as np
import pytest

import ntt_ref
from ntt_ref import CORNERS, EPS, P
from test_batch_checks_cpu import Recorder

OK, POW2, UNS, BAD, DEVICE = 0, 1, 8, 9, 10


# ---- the reference itself ------------------------------------------------------------------------------------------


def test_reference_fast_transform_is_the_definition_at_64():
    rng = random.Random(64)
    for x in ([rng.getrandbits(64) % P for _ in range(64)], [P - 1] * 64, ntt_ref.rows(64, 1, 4)[0]):
        x = [v % P for v in x]
        assert ntt_ref.fast(x) == ntt_ref.direct(x)
        assert ntt_ref.fast(x, inverse=True) == ntt_ref.direct(x, inverse=True)
        assert ntt_ref.fast(ntt_ref.fast(x), inverse=True) == x
    a, b = [rng.getrandbits(64) for _ in range(40)], [rng.getrandbits(64) for _ in range(37)]
    assert ntt_ref.cyclic(a, b, 64) == ntt_ref.cyclic_direct(a, b, 64)  # wraps: 76 > 64


def test_the_stated_facts_hold_in_python_integers():
    assert P == 18446744069414584321 and EPS == 2 ** 64 % P
    for q in (2, 3, 5, 17, 257, 65537):  # the prime factors of p - 1 = 2^32 (2^32 - 1): 7 generates the group
        assert (P - 1) % q == 0 and pow(7, (P - 1) // q, P) != 1
    assert ntt_ref.root(1 << 32) == 1753635133440165772
    assert ntt_ref.root(4) == 2 ** 48 and ntt_ref.root(64) == 2 ** 39
    assert pow(2, 192, P) == 1 and pow(2, 96, P) == P - 1 and all(pow(2, 192 // q, P) != 1 for q in (2, 3))
    assert ntt_ref.root(16384) == 16207902636198568418 and pow(16384, P - 2, P) == 18445618169508003841
    assert ntt_ref.direct(list(range(1, 9))) == [
        36, 18445622567621360637, 18445618169507741693, 1130298020461564, 18446744069414584317, 18445613771394122749,
        1125899906842620, 1121501793223676]


# ---- the field helpers of the C ABI ----------------------------------------------------------------------------------


def test_constants_and_roots(pdsp):
    lib = pdsp.lib
    assert lib.pdsp_ntt_modulus() == P == pdsp.NTT_MODULUS
    assert lib.pdsp_ntt_root(1 << 32) == 1753635133440165772 == pdsp.ntt_root(1 << 32)
    assert lib.pdsp_ntt_root(4) == 2 ** 48 and lib.pdsp_ntt_root(64) == 2 ** 39
    assert lib.pdsp_ntt_root(16384) == 16207902636198568418 and lib.pdsp_ntt_invmod(16384) == 18445618169508003841
    for k in range(0, 33):
        n = 1 << k
        w = lib.pdsp_ntt_root(n)
        assert w == ntt_ref.root(n)
        assert lib.pdsp_ntt_powmod(w, n) == 1
        if k:
            assert lib.pdsp_ntt_powmod(w, n // 2) == P - 1
    for n in (0, -4, 3, 100, 1 << 33):
        assert lib.pdsp_ntt_root(n) == 0
        with pytest.raises(pdsp.PdspError, match=r"^n must be a power of two, 1 \.\.\. 2\^32, got "):
            pdsp.ntt_root(n)


def test_mulmod_on_corner_pairs_and_random_pairs(pdsp):
    lib = pdsp.lib
    assert len(CORNERS) == 15
    for a in CORNERS:
        for b in CORNERS:
            assert lib.pdsp_ntt_mulmod(a, b) == a * b % P, (a, b)
    rng = random.Random(20261019)
    for _ in range(10 ** 4):
        a, b = rng.getrandbits(64), rng.getrandbits(64)
        assert lib.pdsp_ntt_mulmod(a, b) == a * b % P, (a, b)
    # pairs built to take reduce128's borrow and final canon (uniform pairs take either once in 2^32): the host build
    # of the header on the pairs test_gpu_ntt_paths.py puts through ntt_mul_kernel
    import ntt_model
    pairs = ntt_model.targeted_pairs()
    assert {branch for _, _, branch in pairs} == {"borrow", "canon"} and len(pairs) >= 300
    for a, b, _ in pairs:
        assert lib.pdsp_ntt_mulmod(a, b) == a * b % P, (a, b)


def test_invmod_and_powmod(pdsp):
    lib = pdsp.lib
    rng = random.Random(7)
    for a in [v for v in CORNERS if v % P] + [rng.getrandbits(64) for _ in range(200)]:
        inv = lib.pdsp_ntt_invmod(a)
        assert inv < P and lib.pdsp_ntt_mulmod(inv, a) == 1, a
        e = rng.getrandbits(64)
        assert lib.pdsp_ntt_powmod(a, e) == pow(a, e, P)
    assert lib.pdsp_ntt_invmod(0) == 0 and lib.pdsp_ntt_invmod(P) == 0 and lib.pdsp_ntt_powmod(P + 5, 0) == 1


# ---- refusals of the C ABI -----------------------------------------------------------------------------------------


def last(pdsp):
    return pdsp.lib.pdsp_last_error().decode()


@pytest.fixture
def handles(pdsp):
    hs = {}
    for n in (64, 4096, 16384):
        h = C.c_void_p()
        assert pdsp.lib.pdsp_ntt_create(n, -1, C.byref(h)) == OK and pdsp.lib.pdsp_ntt_size(h) == n
        hs[n] = h
    yield hs
    for h in hs.values():
        assert pdsp.lib.pdsp_ntt_destroy(h) == OK


def test_create_refusals(pdsp):
    lib = pdsp.lib
    h = C.c_void_p(1)
    for n in (0, -64, 3, 100, 6 * 1024):
        assert lib.pdsp_ntt_create(n, -1, C.byref(h)) == POW2 and last(pdsp) == f"NTT size must be power of two, got {n}"
        assert not h.value
    for n in (1, 2, 32, 32768, 1 << 20, 1 << 40):
        assert lib.pdsp_ntt_create(n, -1, C.byref(h)) == UNS and last(pdsp) == f"NTT size {n} is outside 64 ... 16384"
    assert lib.pdsp_ntt_create(64, -1, None) == BAD and last(pdsp) == "out is null"
    assert lib.pdsp_ntt_destroy(None) == OK and lib.pdsp_ntt_size(None) == 0
    for n in range(6, 15):
        assert lib.pdsp_ntt_create(1 << n, -1, C.byref(h)) == OK and lib.pdsp_ntt_size(h) == 1 << n
        assert lib.pdsp_ntt_destroy(h) == OK


def no_device(pdsp):
    """Calls that pass every argument check are made only where there is no device to launch on: there they stop at
    PDSP_ERR_DEVICE, which shows that no check refused them.  (With a device they would run on the made-up addresses.)"""
    return pdsp.lib.pdsp_device_count() == 0


A, B_, O = 0x10000000, 0x20000000, 0x30000000  # addresses no refused call ever reads


@pytest.mark.parametrize("fn", ["pdsp_ntt_forward_u64", "pdsp_ntt_inverse_u64"])
def test_transform_refusals(pdsp, handles, fn):
    f = getattr(pdsp.lib, fn)
    h, n = handles[4096], 4096
    cases = [
        ((None, 1, A, n, O, n), "ntt is null"),
        ((h, -1, A, n, O, n), "batch must be >= 0, got -1"),
        ((h, 1, A, n - 1, O, n), f"strides must be >= N = 4096, got {n - 1} (input) and {n} (output)"),
        ((h, 1, A, n, O, 0), f"strides must be >= N = 4096, got {n} (input) and 0 (output)"),
        ((h, 1 << 62, A, n, O, n), f"batch {1 << 62} x stride overflows"),
        ((h, 3, A, 1 << 61, O, n), "batch 3 x stride overflows"),
        ((h, 1, None, n, O, n), "null buffer"),
        ((h, 1, A, n, None, n), "null buffer"),
        ((h, 2, A, n, A + 8, n), "output overlaps input (only out == in with equal strides may share bytes)"),
        ((h, 2, A, n, A, n + 1), "output overlaps input (only out == in with equal strides may share bytes)"),
        ((h, 2, A, n, A + 8 * (2 * n - 1), n), "output overlaps input (only out == in with equal strides may share bytes)"),
    ]
    for (hh, batch, src, ss, dst, ds), text in cases:
        assert f(hh, batch, src, ss, dst, ds, None) == BAD and last(pdsp) == text, text
    # a grid of 2^31 rows (one row per workgroup at N = 16384), checked before the buffers are looked at for overlap
    assert f(handles[16384], 1 << 31, A, 16384, A, 16384, None) == BAD and last(pdsp) == "batch too large: 2147483648"
    assert f(h, 0, None, 0, None, 0, None) == BAD  # strides are checked even for no rows
    assert f(h, 0, None, n, None, n, None) == OK
    if no_device(pdsp):
        assert f(h, 2, A, n, A, n, None) == DEVICE  # the exact in-place call passes every check
        assert f(h, 2, A, n, A + 8 * 2 * n, n, None) == DEVICE  # and so do rows that merely touch


def test_convolution_refusals(pdsp, handles):
    f = pdsp.lib.pdsp_ntt_conv_u64
    h, n = handles[64], 64
    lengths = "lengths must be 1 ... N = 64, got {} (a), {} (b) and {} (out)"
    strides = "strides must be >= the row lengths (b: or 0), got {} (a), {} (b) and {} (out)"
    overlap = "output overlaps an input (only out == a with equal strides may share bytes)"
    cases = [
        ((None, 1, A, 8, 8, B_, 8, 8, O, 8, 8), "ntt is null"),
        ((h, -2, A, 8, 8, B_, 8, 8, O, 8, 8), "batch must be >= 0, got -2"),
        ((h, 1, A, 0, 8, B_, 8, 8, O, 8, 8), lengths.format(0, 8, 8)),
        ((h, 1, A, 65, 65, B_, 8, 8, O, 8, 8), lengths.format(65, 8, 8)),
        ((h, 1, A, 8, 8, B_, 0, 0, O, 8, 8), lengths.format(8, 0, 8)),
        ((h, 1, A, 8, 8, B_, 65, 65, O, 8, 8), lengths.format(8, 65, 8)),
        ((h, 1, A, 8, 8, B_, 8, 8, O, 0, 8), lengths.format(8, 8, 0)),
        ((h, 1, A, 8, 8, B_, 8, 8, O, 65, 65), lengths.format(8, 8, 65)),
        ((h, 1, A, 8, 7, B_, 8, 8, O, 8, 8), strides.format(7, 8, 8)),
        ((h, 1, A, 8, 8, B_, 8, 7, O, 8, 8), strides.format(8, 7, 8)),
        ((h, 1, A, 8, 8, B_, 8, -1, O, 8, 8), strides.format(8, -1, 8)),
        ((h, 1, A, 8, 8, B_, 8, 8, O, 9, 8), strides.format(8, 8, 8)),
        ((h, 1 << 61, A, 8, 8, B_, 8, 0, O, 8, 8), f"batch {1 << 61} x stride overflows"),
        ((h, 4, A, 8, 8, B_, 8, 1 << 61, O, 8, 8), "batch 4 x stride overflows"),
        ((h, 1, None, 8, 8, B_, 8, 8, O, 8, 8), "null buffer"),
        ((h, 1, A, 8, 8, None, 8, 8, O, 8, 8), "null buffer"),
        ((h, 1, A, 8, 8, B_, 8, 8, None, 8, 8), "null buffer"),
        ((h, 2, A, 8, 8, B_, 8, 8, A + 8, 8, 8), overlap),
        ((h, 2, A, 8, 8, B_, 8, 8, A, 8, 9), overlap),
        ((h, 2, A, 8, 8, B_, 8, 8, B_, 8, 8), overlap),       # out == b is not the in-place case
        ((h, 2, A, 8, 8, B_, 8, 0, B_ + 56, 8, 8), overlap),  # one byte range of the shared b row
    ]
    for args, text in cases:
        assert f(*args, None) == BAD and last(pdsp) == text, text
    # 2^31 workgroups: sixteen rows each at N = 64 (16 points per thread, 64 threads)
    assert f(h, 1 << 35, A, 1, 1, B_, 1, 0, O, 1, 1, None) == BAD and last(pdsp) == f"batch too large: {1 << 35}"
    assert f(h, (1 << 35) - 16, A, 1, 1, B_, 1, 0, O, 1, 1, None) == BAD and last(pdsp) == overlap  # the grid fits
    assert f(h, 0, None, 8, 8, None, 8, 8, None, 8, 8, None) == OK
    if no_device(pdsp):
        assert f(h, 2, A, 8, 8, B_, 8, 8, A, 8, 8, None) == DEVICE  # out == a, equal strides
        assert f(h, 2, A, 64, 64, B_, 1, 0, O, 64, 64, None) == DEVICE


def test_mul_refusals(pdsp):
    f = pdsp.lib.pdsp_ntt_mul_u64
    for args, text in (((-1, A, B_, O), "count must be >= 0, got -1"),
                       ((1 << 61, A, B_, O), f"count {1 << 61} overflows"),
                       ((4, None, B_, O), "null buffer"), ((4, A, None, O), "null buffer"), ((4, A, B_, None), "null buffer"),
                       ((4, A, B_, A + 8), "output overlaps input"), ((4, A, B_, B_ - 8), "output overlaps input")):
        assert f(*args, None) == BAD and last(pdsp) == text, text
    assert f(0, None, None, None, None) == OK
    if no_device(pdsp):  # out == a and out == b are exact in place
        assert f(4, A, B_, A, None) == DEVICE and f(4, A, B_, B_, None) == DEVICE and f(4, A, A, A, None) == DEVICE


def test_host_form_refusals(pdsp):
    from pragma_dsp_amd import _capi
    for fn in (pdsp.ntt, pdsp.intt):
        for x, code, text in ((np.zeros(100, np.uint64), POW2, "NTT size must be power of two, got 100"),
                              (np.zeros((2, 0), np.uint64), POW2, "NTT size must be power of two, got 0"),
                              (np.zeros(32, np.int64), UNS, "NTT size 32 is outside 64 ... 16384"),
                              (np.zeros((1, 32768), np.uint64), UNS, "NTT size 32768 is outside 64 ... 16384"),
                              (np.zeros(64), BAD, "input must be an array of uint64 or int64, got float64"),
                              (np.uint64(3), BAD, "input must have at least one axis")):
            with pytest.raises(pdsp.PdspError) as e:
                fn(x)
            assert (e.value.code, str(e.value)) == (code, text)
        assert fn(np.zeros((0, 64), np.uint64)).shape == (0, 64)  # no rows: nothing to do, no device needed
    lib, x = pdsp.lib, np.zeros(64, np.uint64)
    p = C.c_void_p(x.ctypes.data)
    assert lib.pdsp_ntt_host_u64(p, -1, 64, 0, p) == BAD and last(pdsp) == "batch must be >= 0, got -1"
    assert lib.pdsp_ntt_host_u64(p, 1 << 50, 64, 0, p) == BAD and last(pdsp) == f"batch {1 << 50} x length overflows"
    assert lib.pdsp_ntt_host_u64(None, 1, 64, 0, p) == BAD and last(pdsp) == "null buffer"
    conv = lib.pdsp_ntt_conv_host_u64
    assert conv(p, 8, p, 8, 0, 1, 100, p, 8) == POW2 and last(pdsp) == "NTT size must be power of two, got 100"
    assert conv(p, 65, p, 8, 0, 1, 64, p, 8) == BAD and last(pdsp) == "lengths must be 1 ... N = 64, got 65 (a), 8 (b) and 8 (out)"
    assert conv(p, 8, p, 8, 0, 1, 64, p, 0) == BAD and last(pdsp) == "lengths must be 1 ... N = 64, got 8 (a), 8 (b) and 0 (out)"
    assert conv(p, 8, None, 8, 1, 1, 64, p, 8) == BAD and last(pdsp) == "null buffer"
    assert conv(p, 8, p, 8, 1, 0, 64, p, 8) == OK
    for a, b, code in ((np.zeros(9000, np.uint64), np.zeros(8000, np.uint64), _capi.ERR_UNSUPPORTED_SIZE),
                       (np.zeros(0, np.uint64), np.zeros(3, np.uint64), BAD)):
        with pytest.raises(pdsp.PdspError) as e:
            pdsp.polymul(a, b)
        assert e.value.code == code and str(e.value) == (f"the product of rows of {a.size} and {b.size} values needs a "
                                                         "transform of 1 ... 16384 points")
    with pytest.raises(pdsp.PdspError, match=r"^b must have a's 2 rows or be one row, got 3$"):
        pdsp.polymul(np.zeros((2, 4), np.uint64), np.zeros((3, 4), np.uint64))
    if lib.pdsp_device_count() == 0:
        with pytest.raises(pdsp.PdspError) as e:
            pdsp.ntt(x)
        assert e.value.code == DEVICE


# ---- the Python layer --------------------------------------------------------------------------------------------------


def test_python_surface_and_handle_refusals(pdsp):
    assert {"Ntt", "ntt_mul", "ntt", "intt", "polymul", "convolve_exact", "NTT_MODULUS", "ntt_root"} <= set(pdsp.__all__)
    for size, code, text in ((100, POW2, "NTT size must be power of two, got 100"),
                             (32, UNS, "NTT size 32 is outside 64 ... 16384"),
                             (1 << 15, UNS, "NTT size 32768 is outside 64 ... 16384")):
        with pytest.raises(pdsp.PdspError) as e:
            pdsp.Ntt(size)
        assert (e.value.code, str(e.value)) == (code, text)  # argument errors come first, with or without a device
    with pytest.raises(pdsp.PdspError, match="^size must be an integer, got 64.0$"):
        pdsp.Ntt(64.0)
    if pdsp.lib.pdsp_device_count() == 0:
        with pytest.raises(pdsp.PdspError) as e:
            pdsp.Ntt(64)
        assert e.value.code == DEVICE


def test_host_operands_never_reach_the_library(pdsp, monkeypatch):
    """Ntt's methods and ntt_mul hand raw pointers over: a tensor that is not 64-bit words on the handle's device is
    refused in Python.  The library is a recorder, so a missing check would show as a recorded call."""
    import importlib

    import torch
    mod = importlib.import_module("pragma_dsp_amd.ntt")
    rec = Recorder()
    monkeypatch.setattr(mod, "lib", rec)
    plan = mod.Ntt.__new__(mod.Ntt)  # a handle that was never opened: no device is needed to be refused
    plan.device, plan.size = torch.device("cuda", 0), 64
    x = torch.zeros((2, 64), dtype=torch.int64)
    calls = [lambda: plan.forward(x), lambda: plan.inverse(x), lambda: plan.convolve(x, x), lambda: plan.forward(x.numpy()),
             lambda: plan.forward(x.to(torch.float64)), lambda: plan.forward(x.to(torch.int32)),
             lambda: mod.ntt_mul(x, x), lambda: mod.ntt_mul(x.to(torch.float64), x), lambda: mod.ntt_mul(x.numpy(), x.numpy())]
    for call in calls:
        with pytest.raises(pdsp.PdspError) as e:
            call()
        assert e.value.code == BAD
    assert rec.calls == []
    monkeypatch.undo()


def test_convolve_exact_bound_at_both_sides_of_2_62(pdsp):
    """min(len a, len b) max|a| max|b| >= 2^62 is refused, in Python integers, before anything else; just below it the
    call goes on (to the device, or to PDSP_ERR_DEVICE without one)."""
    a = np.array([2 ** 31, -5, 7, 1], dtype=np.int64)   # max|a| = 2^31
    b = np.array([-(2 ** 29), 3, 0, 2, 1], dtype=np.int64)  # max|b| = 2^29, min length 4: 4 * 2^31 * 2^29 = 2^62
    with pytest.raises(pdsp.PdspError) as e:
        pdsp.convolve_exact(a, b)
    assert e.value.code == BAD and str(e.value) == (f"min(len a, len b) max|a| max|b| = 4 x {2 ** 31} x {2 ** 29} must be "
                                                    "below 2^62 for an exact int64 result")
    b[0] += 1  # max|b| = 2^29 - 1: below the bound
    try:
        got = pdsp.convolve_exact(a, b)
    except pdsp.PdspError as err:
        assert pdsp.lib.pdsp_device_count() == 0 and err.code == DEVICE
    else:
        want = [sum(int(a[j]) * int(b[i - j]) for j in range(4) if 0 <= i - j < 5) for i in range(8)]
        assert got.dtype == np.int64 and got.tolist() == want
    big = np.array([2 ** 63 - 1], dtype=np.int64)
    with pytest.raises(pdsp.PdspError):
        pdsp.convolve_exact(big, big)  # computed in Python integers: no wrap hides it
    with pytest.raises(pdsp.PdspError, match="^a must be an array of integers with at least one axis, got float64$"):
        pdsp.convolve_exact(np.zeros(4), b)


# ---- header <-> ctypes ---------------------------------------------------------------------------------------------


def test_header_and_ctypes_symbols_agree(pdsp):
    from test_capi_cpu import header_symbols
    pub = [s for s in header_symbols() if s.startswith("pdsp_ntt_")]
    assert sorted(pub) == sorted([
        "pdsp_ntt_create", "pdsp_ntt_destroy", "pdsp_ntt_size", "pdsp_ntt_forward_u64", "pdsp_ntt_inverse_u64",
        "pdsp_ntt_conv_u64", "pdsp_ntt_mul_u64", "pdsp_ntt_host_u64", "pdsp_ntt_conv_host_u64", "pdsp_ntt_modulus",
        "pdsp_ntt_root", "pdsp_ntt_mulmod", "pdsp_ntt_powmod", "pdsp_ntt_invmod"])
    raw = C.CDLL(pdsp.LIB_PATH)
    for s in pub:
        assert s in pdsp.lib._pdsp_symbols and hasattr(raw, s), s

"""Polyphase rate change without a GPU: the reference the device tests use (a plain restatement of the definition --
zero-stuff, np.convolve, pick every down-th sample -- that shares nothing with the kernel's polyphase structure),
pinned to scipy.signal.resample_poly / upfirdn; the default filter design against scipy.signal.firwin; the
output-length helpers and the gcd reduction; and every refusal the library makes before it needs a device."""
import ctypes as C
import math

import numpy as np
import pytest

import pragma_dsp_amd as pd
from pragma_dsp_amd import _capi
from pragma_dsp_amd._capi import lib

CASES = [(2, 1, 64), (1, 2, 65), (3, 2, 100), (160, 147, 500), (147, 160, 333), (1, 8, 1000), (7, 1, 5), (5, 7, 1),
         (4, 6, 97), (1, 400, 5000), (3, 1, 2)]


def resample_ref(x, up, down, h, t0, y_len, abs=False):  # noqa: A002
    """y[m] = sum_k h[m down + t0 - k up] x[k] in f64, rows along the last axis: zero-stuff, convolve, pick
    t0 + m down.  abs=True: A[m] = sum |h| |x| over the same terms."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    h = np.asarray(h, dtype=np.float64)
    if abs:
        x, h = np.abs(x), np.abs(h)
    rows, n = x.shape
    y = np.zeros((rows, y_len))
    pick = t0 + np.arange(y_len, dtype=np.int64) * down
    for r in range(rows):
        z = np.zeros((n - 1) * up + 1)
        z[::up] = x[r]
        full = np.convolve(z, h)
        ok = pick < full.size
        y[r, ok] = full[pick[ok]]
    return y


def resample_ref_direct(x, up, down, h, t0, y_len, abs=False):  # noqa: A002
    """The same sum in its gather form, for ratios at which the stuffed signal is out of reach (up = 8191):
    y[m] = sum_{j < T} h[p + j up] x[k0 - j], q = m down + t0, p = q mod up, k0 = q div up, T = ceil(ntaps / up), in
    f64, j ascending, all m at once.  Pinned to resample_ref below."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    h = np.asarray(h, dtype=np.float64)
    if abs:
        x, h = np.abs(x), np.abs(h)
    rows, n = x.shape
    q = t0 + np.arange(y_len, dtype=np.int64) * down
    p, k0 = q % up, q // up
    y = np.zeros((rows, y_len))
    for j in range(-(-h.size // up)):
        tap, k = p + j * up, k0 - j
        ok = (tap < h.size) & (k >= 0) & (k < n)
        y[:, ok] += h[tap[ok]] * x[:, k[ok]]
    return y


def poly_setup(up, down, taps=None):
    """(up, down, h, t0) as scipy.signal.resample_poly sets them up; the default taps come from the library's design
    (pinned to scipy.signal.firwin below)."""
    g = math.gcd(up, down)
    up, down = up // g, down // g
    if up == down:
        h = np.ones(1)
    elif taps is None:
        h = pd.design_taps(up, down)
    else:
        h = np.asarray(taps, dtype=np.float64) * up
    return up, down, h, (h.size - 1) // 2


def user_taps(n):
    rng = np.random.default_rng(n)
    return rng.standard_normal(n) / n


def last_error():
    return lib.pdsp_last_error().decode()


@pytest.mark.parametrize("taps", [None, 17, 16], ids=["default", "taps17", "taps16"])
@pytest.mark.parametrize("up,down,n", CASES)
def test_reference_is_scipys_resample_poly(up, down, n, taps):
    ss = pytest.importorskip("scipy.signal")
    x = np.random.default_rng(up * 1000 + down + n).standard_normal(n)
    w = None if taps is None else user_taps(taps)
    want = ss.resample_poly(x, up, down) if w is None else ss.resample_poly(x, up, down, window=w)
    u, d, h, t0 = poly_setup(up, down, w)
    got = resample_ref(x, u, d, h, t0, -(-n * u // d))[0]
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("taps", [17, 16])
@pytest.mark.parametrize("up,down,n", CASES)
def test_reference_is_scipys_upfirdn(up, down, n, taps):
    ss = pytest.importorskip("scipy.signal")
    x = np.random.default_rng(up * 1000 + down + n).standard_normal(n)
    h = user_taps(taps)
    want = ss.upfirdn(h, x, up, down)
    got = resample_ref(x, up, down, h, 0, ((n - 1) * up + taps - 1) // down + 1)[0]
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max()


@pytest.mark.parametrize("taps", [17, 16])
@pytest.mark.parametrize("up,down,n", CASES)
def test_direct_reference_is_the_stuffed_one(up, down, n, taps):
    """Both are f64 sums of the same at most T non-zero terms, each off its exact value by at most T u A[m]:
    |direct - stuffed| <= T 2^-52 A[m], and exactly 0 where no term exists."""
    x = np.random.default_rng(up * 1000 + down + n).standard_normal((2, n))
    h = user_taps(taps)
    t = -(-taps // up)
    for t0 in (0, 1, up, taps + up - 1):
        natural = max(-(-((n - 1) * up + taps - t0) // down), 0)
        for y_len in (max(natural // 2, 1), natural + 10):
            want = resample_ref(x, up, down, h, t0, y_len)
            a = resample_ref(x, up, down, h, t0, y_len, abs=True)
            got = resample_ref_direct(x, up, down, h, t0, y_len)
            assert got.shape == want.shape == (2, y_len)
            assert np.all(np.abs(got - want) <= t * 2.0 ** -52 * a), (t0, y_len)
            assert np.all(got[a == 0] == 0.0) and np.all(want[a == 0] == 0.0)
            assert np.array_equal(resample_ref_direct(x, up, down, h, t0, y_len, abs=True) == 0, a == 0)
            if y_len > natural:
                assert np.all(got[:, natural:] == 0.0)


@pytest.mark.parametrize("up,down", sorted({(u, d) for u, d, _ in CASES}))
def test_design_is_scipys_firwin(up, down):
    ss = pytest.importorskip("scipy.signal")
    g = math.gcd(up, down)
    u, d = up // g, down // g
    m = max(u, d)
    want = ss.firwin(20 * m + 1, 1.0 / m, window=("kaiser", 5.0)) * u
    got = pd.design_taps(up, down)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max()


def test_design_refuses_a_filter_beyond_the_tap_limit():
    n = C.c_longlong(-1)
    assert lib.pdsp_resample_design_f64(8192, 1, None, C.byref(n)) == _capi.ERR_UNSUPPORTED_SIZE
    assert "163841" in last_error() and n.value == -1
    with pytest.raises(pd.PdspError) as e:
        pd.design_taps(8192, 1)
    assert e.value.code == _capi.ERR_UNSUPPORTED_SIZE


def make(poly, up, down, taps=None, t0=0):
    h = C.c_void_p()
    tp = None if taps is None else _capi.dptr(taps)
    nt = 0 if taps is None else taps.size
    rc = (lib.pdsp_resampler_create_poly(-1, up, down, tp, nt, C.byref(h)) if poly
          else lib.pdsp_resampler_create(-1, up, down, tp, nt, t0, C.byref(h)))
    return rc, h


@pytest.mark.parametrize("up,down,n", CASES + [(6, 6, 10)])
def test_output_lengths_and_gcd_reduction(up, down, n):
    g = math.gcd(up, down)
    rc, h = make(True, up, down)
    assert rc == 0
    try:
        u, d = lib.pdsp_resampler_up(h), lib.pdsp_resampler_down(h)
        assert (u, d) == (up // g, down // g)
        nt = lib.pdsp_resampler_ntaps(h)
        assert nt == (1 if u == d else 20 * max(u, d) + 1) and lib.pdsp_resampler_t0(h) == (nt - 1) // 2
        y = C.c_longlong()
        for length in (1, n):
            assert lib.pdsp_resample_output_len(h, length, 0, C.byref(y)) == 0 and y.value == -(-length * u // d)
            assert lib.pdsp_resample_output_len(h, length, 1, C.byref(y)) == 0
            assert y.value == ((length - 1) * u + nt - 1) // d + 1
    finally:
        lib.pdsp_resampler_destroy(h)
    taps = user_taps(17)
    rc, h = make(False, up, down, taps)  # the primitive does not reduce
    assert rc == 0
    try:
        assert (lib.pdsp_resampler_up(h), lib.pdsp_resampler_down(h), lib.pdsp_resampler_ntaps(h)) == (up, down, 17)
        back = np.zeros(17)
        assert lib.pdsp_resampler_taps(h, _capi.dptr(back)) == 0 and np.array_equal(back, taps)
    finally:
        lib.pdsp_resampler_destroy(h)


def test_gcd_reduction_of_4_6():
    rc, h = make(True, 4, 6)
    assert rc == 0 and (lib.pdsp_resampler_up(h), lib.pdsp_resampler_down(h)) == (2, 3)
    lib.pdsp_resampler_destroy(h)


BAD, UNSUP = _capi.ERR_BAD_ARG, _capi.ERR_UNSUPPORTED_SIZE


@pytest.mark.parametrize("up,down,ntaps,code", [
    (0, 1, 17, BAD), (-1, 1, 17, BAD), (1, 0, 17, BAD), (1, -3, 17, BAD), (2, 1, 0, BAD), (2, 1, -1, BAD),
    (8193, 1, 17, UNSUP), (1, 8193, 17, UNSUP), (2, 1, 8193, UNSUP)])
def test_create_refuses(up, down, ntaps, code):
    taps = np.ones(max(ntaps, 1))
    for poly in (False, True):
        h = C.c_void_p(1)
        tp = _capi.dptr(taps)
        rc = (lib.pdsp_resampler_create_poly(-1, up, down, tp, ntaps, C.byref(h)) if poly
              else lib.pdsp_resampler_create(-1, up, down, tp, ntaps, 0, C.byref(h)))
        assert rc == code and last_error() and not h.value


def test_create_refuses_null_and_a_bad_t0():
    taps = np.ones(5)
    h = C.c_void_p(1)
    assert lib.pdsp_resampler_create(-1, 2, 1, None, 5, 0, C.byref(h)) == BAD and last_error() and not h.value
    assert lib.pdsp_resampler_create(-1, 2, 1, _capi.dptr(taps), 5, 0, None) == BAD and last_error()
    assert lib.pdsp_resampler_create_poly(-1, 2, 1, None, 0, None) == BAD and last_error()
    for t0 in (-1, 7):
        assert lib.pdsp_resampler_create(-1, 2, 1, _capi.dptr(taps), 5, t0, C.byref(h)) == BAD and last_error()
        assert not h.value


def test_calls_refuse_before_any_device_work():
    rc, h = make(True, 3, 2)
    assert rc == 0
    try:
        y = C.c_longlong(-7)
        for length in (0, -1):
            assert lib.pdsp_resample_output_len(h, length, 0, C.byref(y)) == BAD and last_error() and y.value == -7
        assert lib.pdsp_resample_output_len(None, 5, 0, C.byref(y)) == BAD and last_error()
        assert lib.pdsp_resample_output_len(h, 5, 0, None) == BAD and last_error()
        buf = np.full(64, 7.0)
        p = C.c_void_p(buf.ctypes.data)
        for fn in (lib.pdsp_upfirdn_f32, lib.pdsp_upfirdn_f64):
            assert fn(None, 1, p, 8, 8, p, 12, 12, None) == BAD and last_error()
            assert fn(h, 1, p, 0, 8, p, 12, 12, None) == BAD and last_error()      # len 0
            assert fn(h, 1, p, -4, 8, p, 12, 12, None) == BAD and last_error()
            assert fn(h, -1, p, 8, 8, p, 12, 12, None) == BAD and last_error()
            assert fn(h, 1, p, 8, 8, p, -1, 12, None) == BAD and last_error()
            assert fn(h, 2, p, 8, 7, p, 12, 12, None) == BAD and last_error()      # x_stride < len
            assert fn(h, 2, p, 8, 8, p, 12, 11, None) == BAD and last_error()      # y_stride < y_len
            assert fn(h, 1, None, 8, 8, p, 12, 12, None) == BAD and last_error()
            assert fn(h, 1, p, 8, 8, None, 12, 12, None) == BAD and last_error()
            assert fn(h, 1, p, 8, 8, p, 12, 12, None) == BAD and "overlaps" in last_error()
        assert np.all(buf == 7.0)
    finally:
        lib.pdsp_resampler_destroy(h)


def test_host_forms_refuse_before_they_write():
    x, y = np.ones(8), np.full(64, 7.0)
    taps = np.ones(5)
    X, Y, H = _capi.dptr(x), _capi.dptr(y), _capi.dptr(taps)
    calls = [
        (lambda: lib.pdsp_resample_poly_host_f64(X, 1, 8, 0, 1, None, 0, Y), BAD),
        (lambda: lib.pdsp_resample_poly_host_f64(X, 1, 8, 1, -1, None, 0, Y), BAD),
        (lambda: lib.pdsp_resample_poly_host_f64(X, 1, 8, 8193, 1, None, 0, Y), UNSUP),
        (lambda: lib.pdsp_resample_poly_host_f64(X, 1, 8, 410, 1, None, 0, Y), UNSUP),   # 8201 default taps
        (lambda: lib.pdsp_resample_poly_host_f64(X, 1, 8, 2, 1, H, 0, Y), BAD),
        (lambda: lib.pdsp_resample_poly_host_f64(X, 1, 8, 2, 1, H, 8193, Y), UNSUP),
        (lambda: lib.pdsp_resample_poly_host_f64(X, 1, 0, 2, 1, None, 0, Y), BAD),
        (lambda: lib.pdsp_resample_poly_host_f64(X, -1, 8, 2, 1, None, 0, Y), BAD),
        (lambda: lib.pdsp_resample_poly_host_f64(None, 1, 8, 2, 1, None, 0, Y), BAD),
        (lambda: lib.pdsp_resample_poly_host_f64(X, 1, 8, 2, 1, None, 0, None), BAD),
        (lambda: lib.pdsp_upfirdn_host_f64(H, 0, X, 1, 8, 1, 1, Y), BAD),
        (lambda: lib.pdsp_upfirdn_host_f64(H, 8193, X, 1, 8, 1, 1, Y), UNSUP),
        (lambda: lib.pdsp_upfirdn_host_f64(None, 5, X, 1, 8, 1, 1, Y), BAD),
        (lambda: lib.pdsp_upfirdn_host_f64(H, 5, X, 1, 8, 0, 1, Y), BAD),
        (lambda: lib.pdsp_upfirdn_host_f64(H, 5, X, 1, 8, 1, 8193, Y), UNSUP),
        (lambda: lib.pdsp_upfirdn_host_f64(H, 5, X, 1, -2, 1, 1, Y), BAD),
        (lambda: lib.pdsp_upfirdn_host_f64(H, 5, None, 1, 8, 1, 1, Y), BAD),
    ]
    for call, code in calls:
        assert call() == code and last_error()
    assert np.all(y == 7.0)


@pytest.mark.parametrize("bad", [2.5, "3", None, True, 2 ** 70])
def test_python_refuses_a_non_integer_ratio(bad):
    for call in (lambda: pd.Resampler(bad, 1), lambda: pd.Resampler(1, bad), lambda: pd.Upfirdn(np.ones(3), bad, 1),
                 lambda: pd.resamplePoly(np.ones(8), bad, 1), lambda: pd.upfirdnHost(np.ones(3), np.ones(8), 1, bad),
                 lambda: pd.design_taps(bad, 1)):
        with pytest.raises(pd.PdspError) as e:
            call()
        assert e.value.code == BAD and "must be an integer" in str(e.value)


def test_python_host_forms_pass_the_librarys_refusals_on():
    for call, code in ((lambda: pd.resamplePoly(np.ones(8), 0, 1), BAD), (lambda: pd.resamplePoly(np.ones(8), 1, 0), BAD),
                       (lambda: pd.resamplePoly(np.ones(8), 8193, 1), UNSUP),
                       (lambda: pd.upfirdnHost(np.ones(8193), np.ones(8)), UNSUP),
                       (lambda: pd.upfirdnHost(np.ones(0), np.ones(8)), BAD),
                       (lambda: pd.resamplePoly(np.ones((2, 0)), 2, 1), BAD)):
        with pytest.raises(pd.PdspError) as e:
            call()
        assert e.value.code == code and str(e.value)

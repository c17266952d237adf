"""The sliding DFT without a GPU (include/pdsp_hip.h, "sliding DFT"): the bindings of every layer, the window identity
behind the components against pdsp_window_make, the exact phase rule of the tables, every refusal of
pdsp_sdft_create(device = -1) with its text, and the numpy emulation of the kernel's summation order (sdft_ref.emulate)
against long double direct sums (sdft_ref.direct) on the shapes the GPU tests run.

Measured here (units of u sqrt(N) max|x|, u = 2^-24 / 2^-53; worst over sizes, lengths, hops, bins and windows):
emulate() 2.23 (f32) and 2.21 (f64); a chunk scanned sequentially 13.2 / 35.2 / 69.5 (f32) and 9.3 / 14.6 / 23.3 (f64)
at N = 1000 / 4096 / 16384.  The device's bound, sdft_ref.BOUND, is four times the former and below the latter.
"""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import sdft_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "pragma-dsp_amd", "js")
SYMBOLS = ("pdsp_sdft_create", "pdsp_sdft_destroy", "pdsp_sdft_length", "pdsp_sdft_bins", "pdsp_sdft_bin", "pdsp_sdft_hop",
           "pdsp_sdft_components", "pdsp_sdft_frames", "pdsp_sdft_f32", "pdsp_sdft_f64", "pdsp_sdft_host_f64",
           "pdsp_sdft_window_weights", "pdsp_sdft_phase_table")
WIN = {"rect": 0, "hann": 1, "hamming": 2, "blackman": 3}


def _create(lib, n, bins, hop=1, win=0, nbins=None):
    from pragma_dsp_amd import _capi
    h = C.c_void_p(0xDEAD)
    b = None if bins is None else np.ascontiguousarray(bins, dtype=np.float64)
    rc = lib.pdsp_sdft_create(n, (0 if b is None else b.size) if nbins is None else nbins, _capi.dptr(b), hop, win, -1,
                              C.byref(h))
    assert h.value == 0xDEAD or rc == 0, "out was touched by a refused call"
    if rc == 0:
        lib.pdsp_sdft_destroy(h)
    return rc, lib.pdsp_last_error()


def _table(lib, n, b, c=0):
    from pragma_dsp_amd import _capi
    re, im = np.empty(n + 1), np.empty(n + 1)
    assert lib.pdsp_sdft_phase_table(n, float(b), c, _capi.dptr(re), _capi.dptr(im)) == 0, lib.pdsp_last_error()
    return re, im


# ---- bindings -------------------------------------------------------------------------------------------------------

def test_capi_declares_the_sdft_symbols(pdsp):
    syms = set(pdsp.lib._pdsp_symbols)
    header = open(os.path.join(ROOT, "include", "pdsp_hip.h")).read()
    declared = set(re.findall(r"PDSP_API\s+[\w\s\*]+?\b(pdsp_sdft_\w+)\s*\(", header))
    assert declared == set(SYMBOLS)
    raw = C.CDLL(pdsp.LIB_PATH)
    for name in SYMBOLS:
        assert name in syms and hasattr(raw, name), name
    assert "typedef struct pdsp_sdft pdsp_sdft;" in header
    for name in ("SlidingDft", "sliding_dft", "goertzel"):
        assert name in pdsp.__all__ and callable(getattr(pdsp, name))
    assert callable(pdsp.SlidingDft.forward) and callable(pdsp.SlidingDft.frames)
    from pragma_dsp_amd import _device
    assert issubclass(pdsp.SlidingDft, _device.Handle)


def test_js_declarations_match_sdft_exports():
    declared = set(re.findall(r"^export function (\w+)", open(os.path.join(JS, "sdft.d.ts")).read(), re.M))
    src = open(os.path.join(JS, "sdft.js")).read()
    body = re.search(r"module\.exports\s*=\s*\{(.*?)\};", src, re.S).group(1)
    assert declared == {p.strip() for p in body.split(",") if p.strip()} == {"slidingDft", "goertzel"}
    idx = open(os.path.join(JS, "index.d.ts")).read()
    assert re.search(r"export const sdft: \{\s*slidingDft: typeof sdftNs\.slidingDft;\s*goertzel: typeof "
                     r"sdftNs\.goertzel;\s*\};", idx)
    js = open(os.path.join(JS, "index.js")).read()
    assert re.search(r"\['sdft', \{ slidingDft: sdft\.slidingDft, goertzel: sdft\.goertzel \}\],", js)   # a row of the table
    assert re.search(r"for \(const \[name, value\] of hidden\) Object\.defineProperty\(module\.exports, name, \{ value, "
                     r"enumerable: false \}\);", js)
    napi = open(os.path.join(ROOT, "pragma-dsp_amd", "csrc", "pdsp_napi.c")).read()
    assert '{"sdft", Sdft}' in napi and "pdsp_sdft_host_f64(" in napi


# ---- the window identity --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 3, 50, 4096])
@pytest.mark.parametrize("win", list(WIN))
def test_components_add_up_to_the_window(pdsp, win, n):
    """w[n] e^(-2 pi i b n / N) = sum over the components of weight x table entry, at every n: the windowed bin is the
    weighted sum of 1, 3 or 5 rectangular sums.  Against pdsp_window_make's f64 window, to a few eps."""
    from pragma_dsp_amd import _capi
    lib = pdsp.lib
    w = np.empty(n)
    assert lib.pdsp_window_make(WIN[win], n, _capi.dptr(w)) == 0
    wts = np.empty(5)
    ncomp = lib.pdsp_sdft_window_weights(WIN[win], _capi.dptr(wts))
    assert ncomp == len(R.components(win)) == {"rect": 1, "hann": 3, "hamming": 3, "blackman": 5}[win]
    assert np.array_equal(wts[:ncomp], [wgt for _, wgt in R.components(win)]) and not wts[ncomp:].any()
    assert abs(np.abs(wts).sum() - 1.0) <= 1e-15
    for b in (0.0, 3.0, 12.5, -2.25):
        base = _table(lib, n, b)
        acc = np.zeros(n + 1, dtype=np.complex128)
        for k, (c, wgt) in enumerate(R.components(win)):
            tr, ti = _table(lib, n, b, c)
            acc += wgt * (tr + 1j * ti)
        want = w * (base[0][:n] + 1j * base[1][:n])
        assert np.abs(acc[:n] - want).max() <= 8 * np.finfo(np.float64).eps, (win, n, b)
    assert lib.pdsp_sdft_window_weights(7, _capi.dptr(wts)) == 0
    assert lib.pdsp_last_error() == b"Unsupported window type: 7"


def test_python_window_is_the_librarys(pdsp):
    from pragma_dsp_amd import _capi
    for win in WIN:
        for n in (2, 3, 50, 4096):
            w = np.empty(n)
            assert pdsp.lib.pdsp_window_make(WIN[win], n, _capi.dptr(w)) == 0
            assert np.abs(R.window(win, n).astype(np.float64) - w).max() <= 4 * np.finfo(np.float64).eps


# ---- the phase rule -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 3, 64, 100, 1000, 16384])
def test_tables_are_exact(pdsp, n):
    lib = pdsp.lib
    i = np.arange(n + 1)
    for b in (0, 1, n // 2, n - 1, 5 * n + 3, -3):
        re, im = _table(lib, n, b)
        # integer bins: the exact N-th roots of unity, from the integer (b i) mod N
        a = R.LD(-2) * R.PI * (((b * i) % n).astype(R.LD) / R.LD(n))
        assert np.array_equal(re, np.cos(a).astype(np.float64)) and np.array_equal(im, np.sin(a).astype(np.float64))
        assert re[n] == 1.0 and im[n] == 0.0
    for b in (12.5, 0.1, -3.75, -0.625, 2.0 ** 30 + 0.25, 1e9 + 0.3):
        for c in (0, 1, -1, 2, -2):
            re, im = _table(lib, n, b, c)
            # b and b + N, b - N: the same table, where the sum is exact in f64 (a dyadic b; -0.625 + N changes sign)
            for b2 in (float(b) + n, float(b) - n):
                if Fraction(b2) - Fraction(float(b)) in (n, -n):
                    re2, im2 = _table(lib, n, b2, c)
                    assert np.array_equal(re, re2) and np.array_equal(im, im2), (n, b, b2, c)
            # and the reference's own statement of the rule, entry for entry
            co, si = R.table(n, b, c)
            assert np.array_equal(re, co.astype(np.float64)) and np.array_equal(im, si.astype(np.float64)), (n, b, c)


def test_a_bin_of_one_tenth_is_the_double_nearest_it():
    """0.1 as a double lies 5.55e-18 above 1/10.  The tables follow the double: in long double the phase at the window's
    end differs from the rational's by 2 pi 5.55e-18 = 3.5e-17 rad, measurably (long double resolves 1e-19); rounded to
    f64 the two tables agree except where the difference crosses a rounding boundary."""
    n = 1000
    exact = Fraction(0.1) - Fraction(1, 10)
    assert 5.5e-18 < float(exact) < 5.6e-18
    i = np.arange(n + 1)
    t_double = R.phase_turns(n, 0.1, 0, i)
    t_tenth = ((i % (10 * n)).astype(R.LD)) / R.LD(10 * n)  # (i / 10) / N, below one turn: no reduction needed
    diff = np.abs(t_double - t_tenth).astype(np.float64)
    assert 5.0e-18 < diff[n] < 6.0e-18 and diff.argmax() >= n - 1
    co, si = R.table(n, 0.1)
    a = R.LD(-2) * R.PI * t_tenth
    moved = np.abs(co - np.cos(a)).max()
    assert 1e-17 < float(moved) < 4e-17
    flips = int((co.astype(np.float64) != np.cos(a).astype(np.float64)).sum())
    print(f"SDFT 0.1-vs-1/10 at N = {n}: phase difference {diff[n]:.3e} turns, {flips} of {n + 1} f64 cosines differ")


# ---- refusals -------------------------------------------------------------------------------------------------------

def test_create_refuses_bad_arguments_and_leaves_out_untouched(pdsp):
    from pragma_dsp_amd import _capi
    lib = pdsp.lib
    size, arg = _capi.ERR_UNSUPPORTED_SIZE, _capi.ERR_BAD_ARG
    inf, nan = float("inf"), float("nan")
    one = [1.0]
    for args, code, text in (
            ((1, one), size, b"sliding DFT window length must be 2 ... 16384, got 1"),
            ((0, one), size, b"sliding DFT window length must be 2 ... 16384, got 0"),
            ((-5, one), size, b"sliding DFT window length must be 2 ... 16384, got -5"),
            ((16385, one), size, b"sliding DFT window length must be 2 ... 16384, got 16385"),
            ((64, []), size, b"sliding DFT bins must be 1 ... 256, got 0"),
            ((64, np.zeros(257)), size, b"sliding DFT bins must be 1 ... 256, got 257"),
            ((64, one, 0), arg, b"hop must be >= 1, got 0"),
            ((64, one, -2), arg, b"hop must be >= 1, got -2"),
            ((64, one, 1, 4), arg, b"Unsupported window type: 4"),
            ((64, one, 1, -1), arg, b"Unsupported window type: -1"),
            ((64, [0.0, nan]), arg, b"sliding DFT bins must be finite and below 2^53 in magnitude, got nan at index 1"),
            ((64, [inf]), arg, b"sliding DFT bins must be finite and below 2^53 in magnitude, got inf at index 0"),
            ((64, [1.0, 2.0, -inf]), arg, b"sliding DFT bins must be finite and below 2^53 in magnitude, got -inf at index 2"),
            ((64, [2.0 ** 53]), arg, b"sliding DFT bins must be finite and below 2^53 in magnitude, got 9.0072e+15 at index 0"),
            ((16384, np.zeros(128)), size, b"sliding DFT tables of 128 bins x 1 components x 16385 entries exceed 2^21 entries"),
            ((16384, np.zeros(26), 1, 3), size, b"sliding DFT tables of 26 bins x 5 components x 16385 entries exceed 2^21 entries"),
            ((8192, np.zeros(86), 1, 1), size, b"sliding DFT tables of 86 bins x 3 components x 8193 entries exceed 2^21 entries")):
        rc, msg = _create(lib, *args)
        assert rc == code and msg == text, (args[0], rc, msg)
    rc, msg = _create(lib, 64, None, nbins=3)
    assert rc == arg and msg == b"bins is null"
    b = np.ones(1)
    assert lib.pdsp_sdft_create(64, 1, _capi.dptr(b), 1, 0, -1, None) == arg
    assert lib.pdsp_last_error() == b"out is null"
    if lib.pdsp_device_count() == 0:
        # arguments the library takes reach the device check, and out stays untouched there too
        for args in ((2, one), (16384, np.zeros(127)), (16384, np.zeros(25), 7, 3), (1000, [12.5, -3.0, 2.0 ** 52], 1 << 40, 2)):
            rc, msg = _create(lib, *args)
            assert rc == _capi.ERR_DEVICE and b"no HIP device" in msg, (args[0], msg)


def test_null_handles_and_host_arguments_are_refused_before_any_device_work(pdsp):
    from pragma_dsp_amd import _capi
    lib = pdsp.lib
    vp = C.c_void_p
    for fn in (lib.pdsp_sdft_f32, lib.pdsp_sdft_f64):
        assert fn(None, 1, vp(16), 64, 64, vp(4096), vp(8192), 1, None) == _capi.ERR_BAD_ARG
        assert lib.pdsp_last_error() == b"sdft is null"
    assert lib.pdsp_sdft_destroy(None) == 0
    for get in (lib.pdsp_sdft_length, lib.pdsp_sdft_bins, lib.pdsp_sdft_hop, lib.pdsp_sdft_components):
        assert get(None) == 0
    assert lib.pdsp_sdft_frames(None, 100) == 0 and lib.pdsp_sdft_bin(None, 0) == 0.0
    x, b = np.ones(64), np.ones(1)
    d, bp = _capi.dptr(x), _capi.dptr(b)
    host = lib.pdsp_sdft_host_f64
    for args, code, text in (
            ((d, 1, 64, 1, 1, bp, 1, 0, d, d), _capi.ERR_UNSUPPORTED_SIZE, b"sliding DFT window length must be 2 ... 16384, got 1"),
            ((d, 0, 64, 8, 1, bp, 1, 0, d, d), _capi.ERR_BAD_ARG, b"batch must be >= 1, got 0"),
            ((d, 1, 7, 8, 1, bp, 1, 0, d, d), _capi.ERR_INPUT_LENGTH, b"sliding DFT rows of 7 samples are shorter than the window of 8"),
            ((d, 1 << 40, 1 << 40, 8, 1, bp, 1, 0, d, d), _capi.ERR_BAD_ARG, b"batch 1099511627776 x (1099511627776, 1099511627769) overflows"),
            ((None, 1, 64, 8, 1, bp, 1, 0, d, d), _capi.ERR_BAD_ARG, b"null buffer"),
            ((d, 1, 64, 8, 1, bp, 1, 0, None, d), _capi.ERR_BAD_ARG, b"null buffer"),
            ((d, 1, 64, 8, 1, bp, 1, 0, d, None), _capi.ERR_BAD_ARG, b"null buffer")):
        assert host(*args) == code and lib.pdsp_last_error() == text, (lib.pdsp_last_error(), text)
    re, im = np.empty(9), np.empty(9)
    assert lib.pdsp_sdft_phase_table(8, 1.0, 3, _capi.dptr(re), _capi.dptr(im)) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"component must be -2 ... 2, got 3"
    assert lib.pdsp_sdft_phase_table(1, 1.0, 0, _capi.dptr(re), _capi.dptr(im)) == _capi.ERR_UNSUPPORTED_SIZE


def test_python_forms_refuse_before_any_device_work(pdsp):
    from pragma_dsp_amd import _capi
    x = np.ones(64)
    for make, code, text in (
            (lambda: pdsp.SlidingDft(1, [1.0]), _capi.ERR_UNSUPPORTED_SIZE, "sliding DFT window length must be 2 ... 16384, got 1"),
            (lambda: pdsp.SlidingDft(64, []), _capi.ERR_UNSUPPORTED_SIZE, "sliding DFT bins must be 1 ... 256, got 0"),
            (lambda: pdsp.SlidingDft(64, [1.0], hop=0), _capi.ERR_BAD_ARG, "hop must be >= 1, got 0"),
            (lambda: pdsp.SlidingDft(64, [1.0], window="kaiser"), _capi.ERR_BAD_ARG, "Unsupported window type: kaiser"),
            (lambda: pdsp.SlidingDft(64.5, [1.0]), _capi.ERR_BAD_ARG, "length must be an integer"),
            (lambda: pdsp.SlidingDft(64, [1.0], hop=1.5), _capi.ERR_BAD_ARG, "hop must be an integer"),
            (lambda: pdsp.SlidingDft(64, [1j]), _capi.ERR_BAD_ARG, "bins must be a real number or a vector of real numbers"),
            (lambda: pdsp.SlidingDft(64, [[1.0, 2.0]]), _capi.ERR_BAD_ARG, "bins must be a real number or a vector"),
            (lambda: pdsp.SlidingDft(64, [float("nan")]), _capi.ERR_BAD_ARG, "sliding DFT bins must be finite"),
            (lambda: pdsp.sliding_dft(x, 65, [1.0]), _capi.ERR_INPUT_LENGTH, "sliding DFT rows of 64 samples are shorter than the window of 65"),
            (lambda: pdsp.sliding_dft(x, 16, [1.0], hop=0), _capi.ERR_BAD_ARG, "hop must be >= 1, got 0"),
            (lambda: pdsp.sliding_dft(x, 16, np.zeros(300)), _capi.ERR_UNSUPPORTED_SIZE, "sliding DFT bins must be 1 ... 256, got 300"),
            (lambda: pdsp.goertzel(np.ones(1), [0.0]), _capi.ERR_UNSUPPORTED_SIZE, "sliding DFT window length must be 2 ... 16384, got 1"),
            (lambda: pdsp.goertzel(np.ones(20000), [0.0]), _capi.ERR_UNSUPPORTED_SIZE, "sliding DFT window length must be 2 ... 16384, got 20000")):
        with pytest.raises(pdsp.PdspError) as e:
            make()
        assert e.value.code == code and str(e.value).startswith(text), str(e.value)


def test_frames_rule():
    # F = 1 + floor((T - N) / h): at T = N - 1, N, N + h - 1, N + h
    for n, h in ((64, 1), (100, 7), (1000, 1001), (2, 5)):
        assert [R.frames_of(n, h, t) for t in (n - 1, n, n + h - 1, n + h)] == [0, 1, 1, 2]


# ---- the emulation against direct sums ------------------------------------------------------------------------------

def test_sliding_reference_is_the_direct_sum():
    # sdft_ref.sliding (one long double prefix sum over the row) against the definition, frame by frame
    for n, h, b in ((64, 1, 3.0), (100, 7, 12.5), (1000, 3, 250.0)):
        x = R.signal(n, 3 * n + 7)
        re, im = R.direct(x, n, [b], h)
        sr, si = R.sliding(x, n, b, h)
        assert max(np.abs(sr - re[:, 0]).max(), np.abs(si - im[:, 0]).max()) <= 2.0 ** -58 * np.sqrt(n) * np.abs(x).max()


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n,win", [(n, w) for n in R.SIZES for w in R.windows_of(n)])
def test_emulated_order_against_direct_sums(n, win, dtype):
    worst = 0.0
    for t in R.lengths(n):
        x = R.signal(n, t)
        for h in R.hops(n):
            fr, re, im = R.reference(n, t, h, win)
            got = R.emulate(x, n, R.bins_of(n), h, win, dtype)
            assert got.shape == (R.ROWS, 7, R.frames_of(n, h, t))
            worst = max(worst, R.err_units(got[:, :, fr], re, im, n, dtype, np.abs(x).max()))
    print(f"SDFT emulate {dtype} N={n} {win}: worst {worst:.3f} u sqrt(N) max|x|")
    assert worst <= R.EMULATED_WORST[dtype]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n", [1000, 4096, 16384])
def test_the_bound_stays_below_a_sequential_scan(n, dtype):
    worst = 0.0
    for t in R.lengths(n):
        x = R.signal(n, t)
        fr, re, im = R.reference(n, t, 1, "rect")
        seq = R.emulate(x, n, R.bins_of(n), 1, "rect", dtype, order="sequential")
        worst = max(worst, R.err_units(seq[:, :, fr], re, im, n, dtype, np.abs(x).max()))
    print(f"SDFT sequential {dtype} N={n}: worst {worst:.3f} u sqrt(N) max|x|; the bound is {R.BOUND[dtype]:.2f}")
    assert R.BOUND[dtype] < worst

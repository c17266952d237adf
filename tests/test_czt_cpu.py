"""The chirp-z transform (pdsp_czt_kernel.h) without a GPU: the definition the kernel and its host-built tables
implement, restated in numpy and held against a direct sum with exact phases and against scipy.signal.czt / zoom_fft;
what the C ABI refuses before any device work; and the bindings' symbol lists.

chirp_z() below is the definition of include/pdsp_hip.h word for word: pre[n] = a^-n w^(n^2/2), post[k] = w^(k^2/2),
b[j] = w^(-j^2/2) at index j for j >= 0 and M + j for j < 0, M = max(32, the power of two >= L + K - 1), every phase an
error-free product reduced with fmod before its error term is added (turns()), X = post IFFT_M(FFT_M(x pre) FFT_M(b)).
With M / 2 the circular convolution aliases (test_a_smaller_m_aliases), which pins the M rule and the layout of the
negative lags.

The module also holds the references the device tests share: direct() for any doubles, grid_direct() for step = p / 2^20
and start = q / 2^20, where n k p + n q reduces mod 2^20 in int64 and cos / sin come from one long double table."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "pragma-dsp_amd", "js")

SYMBOLS = ("pdsp_czt_create", "pdsp_czt_destroy", "pdsp_czt_length", "pdsp_czt_bins", "pdsp_czt_conv_size",
           "pdsp_czt_f32", "pdsp_czt_f64", "pdsp_czt_host_f64")
LD = np.longdouble
PI = 4 * np.arctan(LD(1))
GRID = 1 << 20


def conv_size(length, bins):
    """M: the points of the circular convolution."""
    return max(32, 1 << (length + bins - 2).bit_length())


def turns(n, t, mod):
    """(n t) mod `mod` as a long double, the header's rule: p = n t rounded, e = n t - p exactly (Dekker's split of t;
    n is an integer below 2^26), fmod(p) exact, e added after the reduction."""
    n = np.asarray(n, dtype=np.float64)
    p = n * t
    c = 134217729.0 * t
    hi = c - (c - t)
    lo = t - hi
    e = (n * hi - p) + n * lo
    return np.fmod(p, mod).astype(LD) + e.astype(LD)


def cis(turn):
    """exp(2 pi i turn), evaluated in long double, as complex128."""
    a = 2 * PI * np.asarray(turn, dtype=LD)
    return np.cos(a).astype(np.float64) + 1j * np.sin(a).astype(np.float64)


def half_chirp(n, step, sgn):
    """w^(sgn n^2 / 2), w = exp(-2 pi i step): n^2 step reduced mod 2."""
    n = np.asarray(n, dtype=np.int64)
    return cis(-sgn * turns(n * n, step, 2.0) / 2)


def chirp_z(x, bins, step, start=0.0, radius=1.0, m=None):
    """The chirp-z transform of the rows of x in complex128, on transforms of m points (default: the rule)."""
    x = np.asarray(x, np.complex128)
    ln = x.shape[-1]
    m = conv_size(ln, bins) if m is None else m
    n = np.arange(ln, dtype=np.int64)
    pre = np.power(float(radius), -n.astype(np.float64)) * cis(-turns(n, start, 1.0)) * half_chirp(n, step, 1)
    post = half_chirp(np.arange(bins), step, 1)
    u = np.zeros(x.shape[:-1] + (m,), np.complex128)
    u[..., :ln] = x * pre
    b = np.zeros(m, np.complex128)
    j = np.arange(-(ln - 1), bins, dtype=np.int64)
    b[np.where(j < 0, m + j, j) % m] = half_chirp(j, step, -1)  # (% m only for the aliasing test's smaller m)
    return np.fft.ifft(np.fft.fft(u) * np.fft.fft(b))[..., :bins] * post


def direct(x, bins, step, start=0.0, radius=1.0):
    """X[k] = sum_n x[n] radius^-n exp(-2 pi i (n k step + n start)) with exact phases, complex128 accumulation."""
    x = np.asarray(x, np.complex128)
    n = np.arange(x.shape[-1], dtype=np.int64)
    w = cis(-(turns(np.outer(n, np.arange(bins, dtype=np.int64)), step, 1.0) + turns(n, start, 1.0)[:, None]))
    return (x * np.power(float(radius), -n.astype(np.float64))) @ w


_grid = {}


def grid_table():
    """cos and sin of -2 pi i / 2^20, i < 2^20, in long double."""
    if not _grid:
        a = -2 * PI * np.arange(GRID, dtype=LD) / GRID
        _grid["c"], _grid["s"] = np.cos(a), np.sin(a)
    return _grid["c"], _grid["s"]


def grid_direct(x, bins, p, q=0, radius=1.0, extended=True, chunk=1 << 21):
    """The direct sum for step = p / 2^20, start = q / 2^20 (integers): the phase index n k p + n q is reduced mod 2^20
    in int64, cos / sin are read from the long double table, the K columns are evaluated in chunks.  extended: the sums
    run in long double (the f64 reference), else in complex128 on the rounded table values (plenty for f32)."""
    x = np.asarray(x, np.complex128)
    ln = x.shape[-1]
    n = np.arange(ln, dtype=np.int64)
    xs = x * np.power(float(radius), -n.astype(np.float64))
    c, s = grid_table()
    out = np.empty(x.shape[:-1] + (bins,), np.complex128)
    kc = max(1, chunk // ln)
    for k0 in range(0, bins, kc):
        k = np.arange(k0, min(bins, k0 + kc), dtype=np.int64)
        idx = ((np.outer(n, k) % GRID) * (p % GRID) + (n * (q % GRID))[:, None]) % GRID
        wr, wi = c[idx], s[idx]
        if extended:
            xr, xi = xs.real.astype(LD), xs.imag.astype(LD)
            yr = np.einsum("rn,nk->rk", xr, wr) - np.einsum("rn,nk->rk", xi, wi)
            yi = np.einsum("rn,nk->rk", xr, wi) + np.einsum("rn,nk->rk", xi, wr)
            out[..., k0:k0 + len(k)] = yr.astype(np.float64) + 1j * yi.astype(np.float64)
        else:
            out[..., k0:k0 + len(k)] = xs @ (wr.astype(np.float64) + 1j * wi.astype(np.float64))
    return out


def row_err(got, want, x, radius=1.0):
    """e = max_k |got - want| / max(max_k |want|, ||x radius^-n||_2) per row, its maximum over the rows: the norm term
    keeps a row of one or two bins from dividing by a chance-small value."""
    x = np.asarray(x, np.complex128)
    norm = np.linalg.norm(x * np.power(float(radius), -np.arange(x.shape[-1], dtype=np.float64)), axis=-1)
    den = np.maximum(np.abs(want).max(axis=-1), norm)
    return float((np.abs(got - want).max(axis=-1) / np.where(den > 0, den, 1.0)).max())


def gauss(seed, rows, ln):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((rows, ln)) + 1j * rng.standard_normal((rows, ln))


def test_the_m_rule():
    assert [conv_size(*s) for s in ((1, 1), (1, 7), (16, 17), (17, 17), (1000, 1000), (4096, 1), (4096, 2), (8191, 2),
                                    (500, 3000), (4096, 4097), (1, 8192))] == \
        [32, 32, 32, 64, 2048, 4096, 8192, 8192, 4096, 8192, 8192]
    for ln in list(range(1, 70)) + [1000, 4095, 4096, 4097, 8191]:
        for k in list(range(1, 70)) + [1000, 4095, 4096, 4097]:
            if ln + k - 1 > 8192:
                continue
            m = conv_size(ln, k)
            assert m >= ln + k - 1 and m >= 32 and (m == 32 or m // 2 < ln + k - 1) and m & (m - 1) == 0


def test_the_phase_reduction_is_exact():
    """turns() against rational arithmetic: the reduced product carries every bit of n t."""
    rng = np.random.default_rng(1)
    for t in [1.0 / 1000, 0.1, 3.0 / 7, 1e-9, 0.99999, 123.456, -0.3] + list(rng.uniform(-2, 2, 6)):
        for n in [0, 1, 999, 4095 * 4095, 8191 * 8191]:
            for mod in (1.0, 2.0):
                got = turns(n, t, mod)
                hi = float(got)
                diff = abs(Fraction(hi) + Fraction(float(got - LD(hi))) - Fraction(n) * Fraction(t))
                diff -= int(diff / Fraction(mod)) * Fraction(mod)  # equal mod `mod`
                assert min(diff, Fraction(mod) - diff) <= Fraction(2) ** -63 and abs(got) < mod + 1e-9


CASES = [(1, 1), (1, 7), (7, 1), (2, 2), (16, 17), (17, 16), (33, 97), (97, 33), (500, 300), (255, 770), (1000, 1000)]


@pytest.mark.parametrize("ln,bins", CASES)
def test_restatement_against_the_direct_sum(ln, bins):
    x = gauss(ln * 31 + bins, 3, ln)
    for step, start, radius in ((1.0 / 1000, 0.0, 1.0), (0.37 / bins, 0.123, 1.0), (-0.2 / bins, -0.4, 0.999),
                                (0.01, 1e-3, 1.001)):
        want = direct(x, bins, step, start, radius)
        assert row_err(chirp_z(x, bins, step, start, radius), want, x, radius) <= 1e-12
        assert row_err(chirp_z(x.real, bins, step, start, radius), direct(x.real, bins, step, start, radius), x.real,
                       radius) <= 1e-12


# scipy takes w as a complex double, whose angle is off by up to eps / 2 = 1.1e-16 rad; its chirp w^(n^2/2) carries that
# n^2 / 2 times: 5e-12 rad at max(L, K) = 300, the largest size held against it at 1e-11
SCIPY_CASES = [c for c in CASES if max(c) <= 300] + [(300, 200), (200, 300)]


@pytest.mark.parametrize("ln,bins", SCIPY_CASES)
def test_restatement_against_scipy(ln, bins):
    signal = pytest.importorskip("scipy.signal")
    x = gauss(ln * 17 + bins, 3, ln)
    for step, start, radius in ((1.0 / bins, 0.0, 1.0), (0.37 / bins, 0.123, 1.0), (0.2 / bins, 0.4, 0.9995)):
        w, a = np.exp(-2j * np.pi * step), radius * np.exp(2j * np.pi * start)
        assert row_err(chirp_z(x, bins, step, start, radius), signal.czt(x, bins, w, a), x, radius) <= 1e-11
    for fn, fs, endpoint in (([0.1, 0.3], 2.0, False), (0.25, 2.0, True), ([100.0, 150.0], 1000.0, False)):
        if endpoint and bins == 1:
            continue
        f1, f2 = (0.0, fn) if np.isscalar(fn) else fn
        step, start = (f2 - f1) / (fs * (bins - 1 if endpoint else bins)), f1 / fs
        want = signal.zoom_fft(x, fn, bins, fs=fs, endpoint=endpoint)
        assert row_err(chirp_z(x, bins, step, start), want, x) <= 1e-11


def test_grid_reference_is_the_direct_sum():
    x = gauss(3, 2, 300)
    for p, q, radius in ((1 << 10, 0, 1.0), (777, 12345, 1.0), (GRID - 5, GRID - 1, 0.999)):
        want = direct(x, 170, p / GRID, q / GRID, radius)
        for ext in (True, False):
            assert row_err(grid_direct(x, 170, p, q, radius, extended=ext, chunk=300 * 64), want, x, radius) <= 1e-13


@pytest.mark.parametrize("ln,bins", [(12, 6), (6, 12), (40, 26), (26, 40), (700, 326), (326, 700), (3000, 1098)])
def test_a_smaller_m_aliases(ln, bins):
    m = conv_size(ln, bins)
    assert ln + bins - 1 > m // 2 and ln + bins - 1 <= m // 2 + 2
    x = gauss(ln + bins, 3, ln)
    step = 0.37 / bins
    want = direct(x, bins, step, 0.1)
    assert row_err(chirp_z(x, bins, step, 0.1), want, x) <= 1e-12
    assert row_err(chirp_z(x, bins, step, 0.1, m=m // 2), want, x) > 1e-3


def test_zoom_parameters_against_scipy(pdsp):
    signal = pytest.importorskip("scipy.signal")
    import sys
    mod = sys.modules[pdsp.Czt.__module__]  # (the package's `czt` is the function)
    for ln, fn, bins, fs, endpoint in ((64, [0.1, 0.3], None, 2.0, False), (100, 0.5, 37, 2.0, True),
                                       (1000, [100.0, 150.0], 256, 1000.0, False), (33, [0.25, 0.25], 5, 2.0, True)):
        k = ln if bins is None else bins
        step, start = mod._zoom(fn, k, fs, endpoint)
        z = signal.ZoomFFT(ln, fn, k, fs=fs, endpoint=endpoint)
        assert abs(np.exp(-2j * np.pi * step) - z.w) <= 4e-16 and abs(np.exp(2j * np.pi * start) - z.a) <= 4e-16
        pts = pdsp.czt_points(k, step, start)
        assert np.abs(pts - z.points()).max() <= 1e-13
    assert np.abs(pdsp.czt_points(9, 0.11, 0.3, 0.97)
                  - signal.czt_points(9, np.exp(-2j * np.pi * 0.11), 0.97 * np.exp(2j * np.pi * 0.3))).max() <= 1e-14
    assert np.abs(pdsp.czt_points(4, 0.25) - [1, 1j, -1, -1j]).max() <= 1e-18  # quarter turns, reduced exactly


def _create(lib, *args):
    h = C.c_void_p(0x1234)
    rc = lib.pdsp_czt_create(*args, -1, C.byref(h))
    assert h.value == 0x1234  # out is untouched on failure
    return rc, lib.pdsp_last_error()


def test_create_refuses_bad_arguments_and_leaves_out_untouched(pdsp):
    from pragma_dsp_amd import _capi
    lib = pdsp.lib
    inf, nan = float("inf"), float("nan")
    size, arg = _capi.ERR_UNSUPPORTED_SIZE, _capi.ERR_BAD_ARG
    for args, code, text in (
            ((0, 8, 0.1, 0.0, 1.0), size, b"CZT length must be >= 1, got 0"),
            ((-3, 8, 0.1, 0.0, 1.0), size, b"CZT length must be >= 1, got -3"),
            ((8, 0, 0.1, 0.0, 1.0), size, b"CZT bins must be >= 1, got 0"),
            ((8, -1, 0.1, 0.0, 1.0), size, b"CZT bins must be >= 1, got -1"),
            ((4096, 4098, 0.1, 0.0, 1.0), size, b"CZT length + bins - 1 must be <= 8192, got 4096 + 4098 - 1"),
            ((8193, 1, 0.1, 0.0, 1.0), size, b"CZT length + bins - 1 must be <= 8192, got 8193 + 1 - 1"),
            ((1 << 62, 1 << 62, 0.1, 0.0, 1.0), size, b"CZT length + bins - 1 must be <= 8192"),
            ((8, 8, nan, 0.0, 1.0), arg, b"CZT step and start must be finite numbers of turns below 2^53"),
            ((8, 8, 0.1, inf, 1.0), arg, b"CZT step and start must be finite numbers of turns below 2^53"),
            ((8, 8, -inf, 0.0, 1.0), arg, b"CZT step and start must be finite numbers of turns below 2^53"),
            ((8, 8, 0.1, 0.0, 0.0), arg, b"CZT radius must be finite and > 0, got 0"),
            ((8, 8, 0.1, 0.0, -1.0), arg, b"CZT radius must be finite and > 0, got -1"),
            ((8, 8, 0.1, 0.0, inf), arg, b"CZT radius must be finite and > 0, got inf"),
            ((8, 8, 0.1, 0.0, nan), arg, b"CZT radius must be finite and > 0, got nan"),
            ((1000, 8, 0.1, 0.0, 0.95), arg, b"CZT radius^-(L-1) must lie within [2^-64, 2^64], got radius 0.9"),
            ((1000, 8, 0.1, 0.0, 1.05), arg, b"CZT radius^-(L-1) must lie within [2^-64, 2^64], got radius 1.05")):
        rc, msg = _create(lib, *args)
        assert rc == code and msg.startswith(text), (args, rc, msg)
    assert lib.pdsp_czt_create(8, 8, 0.1, 0.0, 1.0, -1, None) == arg
    assert lib.pdsp_last_error() == b"out is null"
    if lib.pdsp_device_count() == 0:
        # arguments the library takes reach the device check, and out stays untouched there too
        for args in ((1, 1, 0.0, 0.0, 1.0), (4096, 4097, 0.1, 0.2, 1.0), (65, 8, 0.1, 0.0, 0.5), (8192, 1, 0.1, 0.0, 1.005)):
            rc, msg = _create(lib, *args)
            assert rc == _capi.ERR_DEVICE and b"no HIP device" in msg, (args, msg)


def test_python_forms_refuse_before_any_device_work(pdsp):
    from pragma_dsp_amd import _capi
    E = pdsp.PdspError
    for make, code, text in (
            (lambda: pdsp.Czt(0, 8, 0.1), _capi.ERR_UNSUPPORTED_SIZE, "CZT length must be >= 1, got 0"),
            (lambda: pdsp.Czt(8, 8190, 0.1), _capi.ERR_UNSUPPORTED_SIZE, "CZT length + bins - 1 must be <= 8192"),
            (lambda: pdsp.Czt(8, 8, float("nan")), _capi.ERR_BAD_ARG, "CZT step and start must be finite"),
            (lambda: pdsp.Czt(8, 8, 0.1, radius=0.0), _capi.ERR_BAD_ARG, "CZT radius must be finite and > 0"),
            (lambda: pdsp.Czt(2.5, 8, 0.1), _capi.ERR_BAD_ARG, "length must be an integer"),
            (lambda: pdsp.Czt(8, 8, 1j), _capi.ERR_BAD_ARG, "step must be a real number"),
            (lambda: pdsp.Czt.zoom(8, [0.1, 0.2, 0.3]), _capi.ERR_BAD_ARG, "fn must be a scalar or a pair"),
            (lambda: pdsp.Czt.zoom(8, 0.5, fs=0.0), _capi.ERR_BAD_ARG, "fs must be finite and non-zero"),
            (lambda: pdsp.czt(np.ones(8), 8, 0.999 * np.exp(-0.1j)), _capi.ERR_BAD_ARG, "spirals are not supported"),
            (lambda: pdsp.czt(np.ones(8), 8, 1.0 + 1e-12), _capi.ERR_BAD_ARG, "spirals are not supported"),
            (lambda: pdsp.czt(np.ones(8), 8190), _capi.ERR_UNSUPPORTED_SIZE, "CZT length + bins - 1 must be <= 8192"),
            (lambda: pdsp.czt(np.ones(0)), _capi.ERR_UNSUPPORTED_SIZE, "CZT length must be >= 1, got 0"),
            (lambda: pdsp.czt(np.ones(8), 0), _capi.ERR_UNSUPPORTED_SIZE, "CZT bins must be >= 1, got 0"),
            (lambda: pdsp.czt(np.ones(8), a=0.0), _capi.ERR_BAD_ARG, "CZT radius must be finite and > 0"),
            (lambda: pdsp.zoom_fft(np.ones(8), 0.5, 8190), _capi.ERR_UNSUPPORTED_SIZE, "CZT length + bins - 1"),
            (lambda: pdsp.zoom_fft(np.ones(8), [0.1, 0.2], 1, endpoint=True), _capi.ERR_BAD_ARG, "fs must be finite")):
        with pytest.raises(E) as e:
            make()
        assert e.value.code == code and str(e.value).startswith(text), str(e.value)


def test_null_handles_are_refused_before_any_device_work(pdsp):
    from pragma_dsp_amd import _capi
    lib = pdsp.lib
    vp = C.c_void_p
    for fn in (lib.pdsp_czt_f32, lib.pdsp_czt_f64):
        assert fn(None, 1, vp(16), vp(32), 8, vp(64), vp(128), 8, None) == _capi.ERR_BAD_ARG
        assert lib.pdsp_last_error() == b"czt is null"
    assert lib.pdsp_czt_destroy(None) == 0
    assert lib.pdsp_czt_length(None) == 0 and lib.pdsp_czt_bins(None) == 0 and lib.pdsp_czt_conv_size(None) == 0
    x = np.ones(8)
    d = _capi.dptr(x)
    assert lib.pdsp_czt_host_f64(None, None, 1, 8, 8, 0.1, 0.0, 1.0, d, d) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"null buffer"
    assert lib.pdsp_czt_host_f64(d, None, 1, 8, 8, 0.1, 0.0, 1.0, None, d) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"null buffer"
    assert lib.pdsp_czt_host_f64(d, None, 0, 8, 8, 0.1, 0.0, 1.0, d, d) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"batch must be >= 1, got 0"
    assert lib.pdsp_czt_host_f64(d, None, 1, 8, 8190, 0.1, 0.0, 1.0, d, d) == _capi.ERR_UNSUPPORTED_SIZE


def test_capi_declares_the_czt_symbols(pdsp):
    syms = set(pdsp.lib._pdsp_symbols)
    header = open(os.path.join(ROOT, "include", "pdsp_hip.h")).read()
    declared = set(re.findall(r"PDSP_API\s+[\w\s\*]+?\b(pdsp_czt_\w+)\s*\(", header))
    assert declared == set(SYMBOLS)
    raw = C.CDLL(pdsp.LIB_PATH)
    for name in SYMBOLS:
        assert name in syms and hasattr(raw, name), name
    assert "typedef struct pdsp_czt pdsp_czt;" in header
    assert not [s for s in declared if s.startswith("pdsp_dft_")]
    for name in ("Czt", "czt", "zoom_fft", "czt_points"):
        assert name in pdsp.__all__ and callable(getattr(pdsp, name))
    assert callable(pdsp.Czt.forward) and callable(pdsp.Czt.zoom) and not hasattr(pdsp.Czt, "inverse")


def _runtime_exports(name):
    src = open(os.path.join(JS, name + ".js")).read()
    body = re.search(r"module\.exports\s*=\s*\{(.*?)\};", src, re.S).group(1)
    return {p.strip().split(":")[0].strip() for p in body.split(",") if p.strip()}


def test_js_declarations_match_czt_exports():
    declared = set(re.findall(r"^export function (\w+)", open(os.path.join(JS, "czt.d.ts")).read(), re.M))
    assert declared == _runtime_exports("czt") == {"czt", "zoomFft"}
    idx = open(os.path.join(JS, "index.d.ts")).read()
    assert re.search(r"export const czt: \{\s*czt: typeof cztNs\.czt;\s*zoomFft: typeof cztNs\.zoomFft;\s*\};", idx)
    js = open(os.path.join(JS, "index.js")).read()
    assert re.search(r"\['czt', \{ czt: czt\.czt, zoomFft: czt\.zoomFft \}\],", js)   # a row of the table of non-enumerable sub-modules
    assert re.search(r"for \(const \[name, value\] of hidden\) Object\.defineProperty\(module\.exports, name, \{ value, "
                     r"enumerable: false \}\);", js)
    napi = open(os.path.join(ROOT, "pragma-dsp_amd", "csrc", "pdsp_napi.c")).read()
    assert napi.count("pdsp_czt_") == 1 and '{"czt", Czt}' in napi  # one binding, of the host form

"""The multi-level wavelet transform without a device: an f64 numpy restatement of the definition in
include/pdsp_hip.h (the reference the GPU tests hold the kernels to), pinned to the explicit n x n analysis matrix and
to the Haar closed form; the built-in Daubechies taps; every refusal with its code and exact text; the header and
ctypes symbols; the tile rule through pdsp_dev_dwt_tile.  Every library call here ends in a refusal or needs no
device: nothing is launched."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the definition, restated in f64 numpy -------------------------------------------------------------------------


def qmf(h):
    """g[j] = (-1)^j h[F - 1 - j]"""
    h = np.asarray(h, dtype=np.float64)
    return h[::-1] * (-1.0) ** np.arange(h.size)


def analysis_level(a, h, g):
    """rows a [..., m] (m even) -> (cA, cD) [..., m / 2]: sum_j h[j] a[(2k + j) mod m], and the same with g"""
    m = a.shape[-1]
    idx = (2 * np.arange(m // 2)[:, None] + np.arange(h.size)[None, :]) % m
    w = a[..., idx]
    return w @ h, w @ g


def synthesis_level(ca, cd, h, g):
    """(cA, cD) [..., m'] -> x [..., 2 m']: x[2i + s] = sum_t h[2t + s] cA[(i - t) mod m'] + g[2t + s] cD[(i - t) mod m']"""
    mp = ca.shape[-1]
    idx = (np.arange(mp)[:, None] - np.arange(h.size // 2)[None, :]) % mp
    wa, wd = ca[..., idx], cd[..., idx]
    x = np.empty((*ca.shape[:-1], 2 * mp))
    x[..., 0::2] = wa @ h[0::2] + wd @ g[0::2]
    x[..., 1::2] = wa @ h[1::2] + wd @ g[1::2]
    return x


def wavedec_ref(x, h, levels, abs=False):
    """[cA_J | cD_J | ... | cD_1] of rows x [..., n]; abs=True: the same recursion with |h|, |g|, |x| (the A of the
    bounds)."""
    h = np.asarray(h, dtype=np.float64)
    g = qmf(h)
    a = np.asarray(x, dtype=np.float64)
    if abs:
        h, g, a = np.abs(h), np.abs(g), np.abs(a)
    out = np.empty_like(a)
    for _ in range(levels):
        m = a.shape[-1]
        assert m % 2 == 0
        a, out[..., m // 2:m] = analysis_level(a, h, g)
    out[..., :a.shape[-1]] = a
    return out


def waverec_ref(c, h, levels, abs=False):
    """rows of samples from rows of coefficients c [..., n] in wavedec_ref's layout; abs=True: |h|, |g|, |c|."""
    h = np.asarray(h, dtype=np.float64)
    g = qmf(h)
    c = np.asarray(c, dtype=np.float64)
    if abs:
        h, g, c = np.abs(h), np.abs(g), np.abs(c)
    m = c.shape[-1] >> levels
    a = c[..., :m]
    for _ in range(levels):
        a = synthesis_level(a, c[..., m:2 * m], h, g)
        m *= 2
    return a


def band_levels(n, levels):
    """The level l of every position of the layout: cD_l -> l, cA_J -> J."""
    lv = np.empty(n)
    m = n
    for l in range(1, levels + 1):
        lv[m // 2:m] = l
        m //= 2
    lv[:m] = levels
    return lv


def lattice_taps(f, seed):
    """An orthonormal scaling filter of f taps that is no Daubechies filter: a paraunitary lattice of f / 2 rotations
    (each step h' = cos t [h, 0, 0] + sin t [0, 0, g] keeps the double-shift orthonormality exactly)."""
    th = np.random.default_rng(seed).uniform(0.2, 1.3, f // 2)
    h = np.array([np.cos(th[0]), np.sin(th[0])])
    for t in th[1:]:
        h = np.cos(t) * np.concatenate([h, [0, 0]]) + np.sin(t) * np.concatenate([[0, 0], qmf(h)])
    return h


def residual(h):
    f = len(h)
    return max(abs(float(np.dot(h[:f - 2 * m], h[2 * m:])) - (m == 0)) for m in range(f // 2))


def level_matrix(m, h, abs=False):
    """The m x m matrix of one level, built entry by entry from the definition: rows 0 ... m/2 - 1 give cA, the rest cD."""
    g = qmf(h)
    if abs:
        h, g = np.abs(h), np.abs(g)
    w = np.zeros((m, m))
    for k in range(m // 2):
        for j in range(len(h)):
            w[k, (2 * k + j) % m] += h[j]
            w[m // 2 + k, (2 * k + j) % m] += g[j]
    return w


def analysis_matrix(n, h, levels, abs=False):
    w = np.eye(n)
    m = n
    for _ in range(levels):
        step = np.eye(n)
        step[:m, :m] = level_matrix(m, h, abs)
        w = step @ w
        m //= 2
    return w


# ---- the restatement against independent forms ---------------------------------------------------------------------

DB2 = np.array([1 + np.sqrt(3), 3 + np.sqrt(3), 3 - np.sqrt(3), 1 - np.sqrt(3)]) / (4 * np.sqrt(2))


@pytest.mark.parametrize("h,levels", [(DB2, 1), (DB2, 3), (lattice_taps(8, 1), 3), (lattice_taps(8, 2), 4),
                                      (lattice_taps(32, 3), 4)], ids=["db2-1", "db2-3", "f8-3", "f8-4", "f32-4"])
def test_reference_is_the_explicit_analysis_matrix(h, levels):
    n = 16  # the 8- and 32-tap filters exceed the deeper levels' lengths: the index wraps more than once
    w = analysis_matrix(n, h, levels)
    assert np.abs(w @ w.T - np.eye(n)).max() <= 1e-14
    x = np.random.default_rng(levels).standard_normal((3, n))
    c = wavedec_ref(x, h, levels)
    assert np.abs(c - x @ w.T).max() <= 1e-14
    assert np.abs(waverec_ref(c, h, levels) - c @ w).max() <= 1e-14
    assert np.abs(waverec_ref(c, h, levels) - x).max() <= 1e-14
    assert abs((c ** 2).sum() - (x ** 2).sum()) <= 1e-13 * (x ** 2).sum()
    # the abs forms are the same matrices with |h[j]|, |g[j]| added up, on |x| and |c|
    wa = analysis_matrix(n, h, levels, abs=True)
    fa, ba = np.abs(x) @ wa.T, np.abs(c) @ wa  # sums of positive terms, which grow with every level: relative
    assert np.abs(wavedec_ref(x, h, levels, abs=True) - fa).max() <= 1e-14 * fa.max()
    assert np.abs(waverec_ref(c, h, levels, abs=True) - ba).max() <= 1e-14 * ba.max()
    assert np.all(wavedec_ref(x, h, levels, abs=True) >= np.abs(c) - 1e-14)


def test_reference_is_the_haar_closed_form():
    x = np.random.default_rng(7).standard_normal((2, 24))
    s = np.sqrt(0.5)
    c = wavedec_ref(x, [s, s], 3)
    a = x
    for l in range(3):
        m = a.shape[-1]
        assert np.abs(c[:, m // 2:m] - s * (a[:, 0::2] - a[:, 1::2])).max() <= 1e-15
        a = s * (a[:, 0::2] + a[:, 1::2])
    assert np.abs(c[:, :3] - a).max() <= 1e-15
    assert np.abs(waverec_ref(c, [s, s], 3) - x).max() <= 1e-15


def test_not_a_power_of_two_and_filters_longer_than_the_level():
    rng = np.random.default_rng(11)
    for h, n, levels in ((lattice_taps(8, 5), 96, 5), (lattice_taps(32, 6), 8, 3), (lattice_taps(20, 7), 4096, 12)):
        x = rng.standard_normal(n)
        c = wavedec_ref(x, h, levels)
        assert np.abs(waverec_ref(c, h, levels) - x).max() <= 1e-13
        assert abs((c ** 2).sum() - (x ** 2).sum()) <= 1e-13 * (x ** 2).sum()
    assert list(band_levels(8, 2)) == [2, 2, 2, 2, 1, 1, 1, 1] and list(band_levels(6, 1)) == [1] * 6


# ---- the built-in wavelets -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", range(1, 11))
def test_builtin_taps(pdsp, p):
    h = pdsp.wavelet_taps(f"db{p}")
    assert h.dtype == np.float64 and h.shape == (2 * p,)
    assert abs(h.sum() - np.sqrt(2)) <= 1e-14
    assert residual(h) <= 1e-14
    # p vanishing moments of g, scaled: the plain sums are ill-conditioned at the high moments of the long filters
    g, j = qmf(h), np.arange(2 * p, dtype=np.float64)
    for q in range(p):
        assert abs((g * j ** q).sum()) <= 1e-9 * (np.abs(g) * j ** q).sum(), (p, q)


def test_builtin_closed_forms(pdsp):
    assert np.array_equal(pdsp.wavelet_taps("haar"), pdsp.wavelet_taps("db1"))
    assert np.abs(pdsp.wavelet_taps("haar") - np.sqrt(0.5)).max() <= 1e-15
    assert np.abs(pdsp.wavelet_taps("db2") - DB2).max() <= 1e-15
    r = np.sqrt(10.0)
    s = np.sqrt(5.0 + 2.0 * r)
    db3 = np.array([1 + r + s, 5 + r + 3 * s, 10 - 2 * r + 2 * s, 10 - 2 * r - 2 * s, 5 + r - 3 * s, 1 + r - s]) / (16 * np.sqrt(2))
    assert np.abs(pdsp.wavelet_taps("db3") - db3).max() <= 1e-15


def test_the_generator_reproduces_the_committed_table(pdsp):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_daubechies
    assert gen_daubechies.MAX_P == 10
    for p in range(1, 11):
        assert np.abs(gen_daubechies.daubechies(p) - pdsp.wavelet_taps(f"db{p}")).max() <= 1e-14, p
    # the table in the host code is the tool's output, line for line
    src = open(os.path.join(ROOT, "pragma-dsp_amd", "csrc", "pdsp_capi_dwt.hip")).read()
    assert gen_daubechies.table() in src


# ---- refusals: code and text, no device ----------------------------------------------------------------------------


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None


def last(pdsp):
    return pdsp.lib.pdsp_last_error().decode()


def create(pdsp, name, taps, levels):
    h = C.c_void_p()
    t = None if taps is None else np.ascontiguousarray(taps, dtype=np.float64)
    rc = pdsp.lib.pdsp_dwt_create(-1, name, dp(t), 0 if t is None else t.size, levels, C.byref(h))
    return rc, h


CREATE_REFUSALS = [
    (b"sym4", None, 3, 'unknown wavelet "sym4" (haar, db1 ... db10)'),
    (b"db11", None, 3, 'unknown wavelet "db11" (haar, db1 ... db10)'),
    (b"db0", None, 3, 'unknown wavelet "db0" (haar, db1 ... db10)'),
    (b"", None, 3, 'unknown wavelet "" (haar, db1 ... db10)'),
    (None, [0.5, 0.5, 0.5], 3, "the scaling filter must have an even number of taps, 2 ... 32, got 3"),
    (None, [], 3, "the scaling filter must have an even number of taps, 2 ... 32, got 0"),
    (None, np.full(34, 0.1), 3, "the scaling filter must have an even number of taps, 2 ... 32, got 34"),
    (None, [0.5, 0.5], 3, "the taps are not an orthonormal scaling filter: sum_k h[k] h[k + 0] is not 1 within 1e-10"),
    (None, [0.5, 0.5, 0.5, 0.5], 3,
     "the taps are not an orthonormal scaling filter: sum_k h[k] h[k + 2] is not 0 within 1e-10"),
    (None, [np.nan, 1.0], 3, "the taps are not an orthonormal scaling filter: sum_k h[k] h[k + 0] is not 1 within 1e-10"),
    (None, DB2 * (1 + 1e-9), 3,
     "the taps are not an orthonormal scaling filter: sum_k h[k] h[k + 0] is not 1 within 1e-10"),
    (b"db2", None, 0, "levels must be >= 1, got 0"),
    (b"db2", None, -4, "levels must be >= 1, got -4"),
    (b"db2", DB2, 3, "pass a wavelet name or taps, not both"),
]


@pytest.mark.parametrize("name,taps,levels,text", CREATE_REFUSALS)
def test_create_refusals(pdsp, name, taps, levels, text):
    from pragma_dsp_amd import _capi
    rc, h = create(pdsp, name, taps, levels)
    assert rc == _capi.ERR_BAD_ARG and not h.value
    assert last(pdsp) == text
    if name is None or taps is None:
        with pytest.raises(pdsp.PdspError) as e:
            pdsp.Dwt(name.decode() if name is not None else taps, levels)
        assert str(e.value) == text and e.value.code == _capi.ERR_BAD_ARG


def test_create_accepts_and_reports(pdsp):
    for name, taps in ((b"db4", None), (None, lattice_taps(6, 4)), (None, lattice_taps(32, 9)), (None, DB2 * (1 + 1e-12))):
        rc, h = create(pdsp, name, taps, 5)
        assert rc == 0, last(pdsp)
        want = pdsp.wavelet_taps(name.decode()) if name else np.asarray(taps)
        assert pdsp.lib.pdsp_dwt_ntaps(h) == want.size and pdsp.lib.pdsp_dwt_levels(h) == 5
        got = np.empty(want.size)
        assert pdsp.lib.pdsp_dwt_taps(h, dp(got)) == 0 and np.array_equal(got, want)
        assert pdsp.lib.pdsp_dwt_destroy(h) == 0
    assert pdsp.lib.pdsp_dwt_destroy(None) == 0 and pdsp.lib.pdsp_dwt_ntaps(None) == 0 and pdsp.lib.pdsp_dwt_levels(None) == 0
    n = C.c_longlong()
    from pragma_dsp_amd import _capi
    assert pdsp.lib.pdsp_wavelet_taps(b"coif1", None, C.byref(n)) == _capi.ERR_BAD_ARG
    assert last(pdsp) == 'unknown wavelet "coif1" (haar, db1 ... db10)'
    assert pdsp.lib.pdsp_wavelet_taps(None, None, C.byref(n)) == _capi.ERR_BAD_ARG and last(pdsp) == "wavelet name is null"
    with pytest.raises(pdsp.PdspError, match=r'^unknown wavelet "sym8" \(haar, db1 \.\.\. db10\)$'):
        pdsp.wavelet_taps("sym8")


@pytest.fixture
def handle(pdsp):
    made = []

    def make(name, levels):
        rc, h = create(pdsp, name, None, levels)
        assert rc == 0
        made.append(h)
        return h

    yield make
    for h in made:
        pdsp.lib.pdsp_dwt_destroy(h)


def call(pdsp, fn, h, batch, x, length, xs, y, ys):
    """x, y: byte addresses (never dereferenced by a refused call) or None."""
    return getattr(pdsp.lib, fn)(h, batch, C.c_void_p(x), length, xs, C.c_void_p(y), ys, None)


@pytest.mark.parametrize("fn,eb", [("pdsp_dwt_forward_f32", 4), ("pdsp_dwt_forward_f64", 8),
                                   ("pdsp_dwt_inverse_f32", 4), ("pdsp_dwt_inverse_f64", 8)])
def test_call_refusals(pdsp, handle, fn, eb):
    from pragma_dsp_amd import _capi
    BAD, UNS = _capi.ERR_BAD_ARG, _capi.ERR_UNSUPPORTED_SIZE
    buf = np.zeros(1 << 18)  # addresses only
    a = buf.ctypes.data
    h3 = handle(b"db2", 3)
    cases = [
        (None, 1, a, 8, 8, a + 4096, 8, BAD, "dwt is null"),
        (h3, -1, a, 8, 8, a + 4096, 8, BAD, "batch must be >= 0, got -1"),
        (h3, 1, a, 0, 8, a + 4096, 8, BAD, "len must be a positive multiple of 2^levels (levels = 3), got 0"),
        (h3, 1, a, -8, 8, a + 4096, 8, BAD, "len must be a positive multiple of 2^levels (levels = 3), got -8"),
        (h3, 1, a, 100, 100, a + 4096, 100, BAD, "len must be a positive multiple of 2^levels (levels = 3), got 100"),
        (h3, 2, a, 8, 4, a + 4096, 8, BAD, "strides must be >= len = 8, got 4 (input) and 8 (output)"),
        (h3, 2, a, 8, 8, a + 4096, 7, BAD, "strides must be >= len = 8, got 8 (input) and 7 (output)"),
        (h3, 1 << 62, a, 8, 1 << 40, a + 4096, 8, BAD, "batch 4611686018427387904 x stride overflows"),
        (h3, 1 << 60, a, 8, 8, a + 4096, 8, BAD, "batch 1152921504606846976 x stride overflows"),
        (h3, 1, None, 8, 8, a + 4096, 8, BAD, "null buffer"),
        (h3, 1, a, 8, 8, None, 8, BAD, "null buffer"),
        (h3, 1 << 31, a, 8, 8, a + (1 << 40), 8, BAD, "batch too large: 2147483648 rows of 1 tiles"),
        # resident rows: only the exact in-place call may share bytes
        (h3, 2, a, 8, 8, a + 4 * eb, 8, BAD, "output overlaps input (only out == in with equal strides may share bytes)"),
        (h3, 2, a, 8, 8, a, 16, BAD, "output overlaps input (only out == in with equal strides may share bytes)"),
        (h3, 2, a, 8, 16, a + 8 * eb, 16, BAD, "output overlaps input (only out == in with equal strides may share bytes)"),
        # rows beyond the resident path: no overlap at all, the exact in-place call included
        (h3, 1, a, 1 << 16, 1 << 16, a, 1 << 16, BAD, "output overlaps input (rows beyond the resident path share no bytes)"),
        (h3, 1, a, 1 << 16, 1 << 16, a + eb, 1 << 16, BAD,
         "output overlaps input (rows beyond the resident path share no bytes)"),
    ]
    for h, batch, x, length, xs, y, ys, code, text in cases:
        assert call(pdsp, fn, h, batch, x, length, xs, y, ys) == code, (text, last(pdsp))
        assert last(pdsp) == text
    # batch 0 is a no-op after the size checks, before the pointers are looked at
    assert call(pdsp, fn, h3, 0, None, 8, 8, None, 8) == 0
    # the depth limit of the tiled path, on a long row
    lim = 32768 // eb
    h11, h13, h14 = handle(b"db4", 11 if eb == 4 else 10), handle(b"haar", 13 if eb == 4 else 12), handle(b"haar", 14 if eb == 4 else 13)
    n = 1 << 16
    if "forward" in fn:  # the inverse's halo does not grow: it would take this call
        assert call(pdsp, fn, h11, 1, a, n, n, a + n * eb, n) == UNS
        assert last(pdsp) == (f"forward DWT of {11 if eb == 4 else 10} levels with 8 taps on rows of 65536: beyond the resident "
                              f"path max(halo, 2^levels) must be <= {lim} values, halo = (taps - 2)(2^levels - 1): at most "
                              f"{10 if eb == 4 else 9} levels")
        assert pdsp.lib.pdsp_dwt_max_levels(8, n, eb) == (10 if eb == 4 else 9)
    if pdsp.lib.pdsp_device_count() == 0:
        assert call(pdsp, fn, h13, 1, a, n, n, a + n * eb, n) == _capi.ERR_DEVICE  # 2^levels == the limit: taken
    rc = call(pdsp, fn, h14, 1, a, n, n, a + n * eb, n)
    assert rc == UNS
    if "forward" in fn:
        assert last(pdsp) == (f"forward DWT of {14 if eb == 4 else 13} levels with 2 taps on rows of 65536: beyond the resident "
                              f"path max(halo, 2^levels) must be <= {lim} values, halo = (taps - 2)(2^levels - 1): at most "
                              f"{13 if eb == 4 else 12} levels")
    else:
        assert last(pdsp) == (f"inverse DWT of {14 if eb == 4 else 13} levels on rows of 65536: beyond the resident path a tile "
                              f"is a multiple of 2^levels, at most {lim} values")


def test_host_form_refusals(pdsp):
    from pragma_dsp_amd import _capi
    x = np.zeros(100)
    for fn in (pdsp.wavedecHost, pdsp.waverecHost):
        for args, text in (((x, "db2", 3), "len must be a positive multiple of 2^levels (levels = 3), got 100"),
                           ((x[:0], "db2", 3), "len must be a positive multiple of 2^levels (levels = 3), got 0"),
                           ((x, "db2", 0), "levels must be >= 1, got 0"),
                           ((x, "sym4", 2), 'unknown wavelet "sym4" (haar, db1 ... db10)'),
                           ((x, [1.0, 0.0, 0.0], 2), "the scaling filter must have an even number of taps, 2 ... 32, got 3")):
            with pytest.raises(pdsp.PdspError) as e:
                fn(*args)
            assert str(e.value) == text and e.value.code == _capi.ERR_BAD_ARG
    with pytest.raises(pdsp.PdspError, match="^levels must be an integer, got 2.5$"):
        pdsp.wavedecHost(x, "db2", 2.5)
    with pytest.raises(pdsp.PdspError) as e:
        pdsp.wavedecHost(np.zeros(1 << 17), "db4", 11)  # f64: 6 * 2047 > 4096
    assert e.value.code == _capi.ERR_UNSUPPORTED_SIZE and "at most 9 levels" in str(e.value)


def test_python_surface(pdsp):
    assert {"Dwt", "wavedec", "waverec", "wavedecHost", "waverecHost", "wavelet_taps"} <= set(pdsp.__all__)

    class Shape:  # split() looks at the last axis only
        levels = 3
    c = np.arange(2 * 24).reshape(2, 24)
    bands = pdsp.Dwt.split(Shape, c)
    assert [b.shape[-1] for b in bands] == [3, 3, 6, 12]
    assert np.array_equal(np.concatenate(bands, axis=-1), c) and all(np.shares_memory(b, c) for b in bands)
    with pytest.raises(pdsp.PdspError, match=r"^len must be a positive multiple of 2\^levels \(levels = 3\), got 20$"):
        pdsp.Dwt.split(Shape, np.zeros(20))


# ---- header <-> ctypes ---------------------------------------------------------------------------------------------


def test_header_and_ctypes_symbols_agree(pdsp):
    from test_capi_cpu import header_symbols
    pub = [s for s in header_symbols() if s.startswith(("pdsp_dwt_", "pdsp_wavelet_"))]
    assert sorted(pub) == sorted([
        "pdsp_dwt_create", "pdsp_dwt_destroy", "pdsp_dwt_ntaps", "pdsp_dwt_levels", "pdsp_dwt_taps", "pdsp_wavelet_taps",
        "pdsp_dwt_max_levels", "pdsp_dwt_forward_f32", "pdsp_dwt_forward_f64", "pdsp_dwt_inverse_f32",
        "pdsp_dwt_inverse_f64", "pdsp_dwt_forward_host_f64", "pdsp_dwt_inverse_host_f64"])
    dev = [s for s in header_symbols("pdsp_hip_dev.h") if "dwt" in s]
    assert sorted(dev) == ["pdsp_dev_dwt_tile", "pdsp_set_dwt_tile"]
    raw = C.CDLL(pdsp.LIB_PATH)
    for s in pub + dev:
        assert s in pdsp.lib._pdsp_symbols and hasattr(raw, s), s


# ---- the tile rule -------------------------------------------------------------------------------------------------


@pytest.fixture
def tile_switch(pdsp):
    prev = pdsp.lib.pdsp_set_dwt_tile(0)
    yield pdsp.lib.pdsp_set_dwt_tile
    pdsp.lib.pdsp_set_dwt_tile(prev)


def tile(pdsp, f, levels, n, eb, inverse):
    info = (C.c_longlong * 5)()
    rc = pdsp.lib.pdsp_dev_dwt_tile(f, levels, n, eb, int(inverse), info)
    return rc, dict(zip(("resident", "tile", "halo", "lds", "tiles"), info))


def expected_lds(f, t, eb, inverse, n):
    """DESIGN.md 4.12"""
    if t["resident"]:
        return (n + n // 2 + (n // 4 if inverse else 0)) * eb
    if inverse:
        return (t["tile"] // 2 * 2 + t["tile"] // 4 + 3 * (f - 2)) * eb
    span = t["tile"] + t["halo"]
    return (span + (span - (f - 2)) // 2) * eb


def test_the_tile_rule(pdsp, tile_switch):
    from pragma_dsp_amd import _capi
    for eb in (4, 8):
        for inverse in (False, True):
            for f in (2, 4, 8, 20, 32):
                for n, levels in ((2, 1), (8, 3), (96, 5), (4096, 12), (4096, 6), (10240, 3), (12288, 4), (1 << 16, 1),
                                  (1 << 16, 4), (3 << 15, 8), (1 << 20, 8), (1 << 20, 6), (1 << 26, 2)):
                    rc, t = tile(pdsp, f, levels, n, eb, inverse)
                    halo = f - 2 if inverse else (f - 2) * ((1 << levels) - 1)
                    lim = 32768 // eb
                    res_values = n + n // 2 + (n // 4 if inverse else 0)
                    if res_values * eb > 65536 and max(halo, 1 << levels) > lim:
                        if res_values * eb <= 163840:  # the resident path takes what the tiled path refuses
                            assert rc == 0 and t["resident"] == 1, (f, n, levels)
                        else:
                            assert rc == _capi.ERR_UNSUPPORTED_SIZE, (f, n, levels)
                        continue
                    assert rc == 0, (f, n, levels, last(pdsp))
                    assert t["resident"] == (res_values * eb <= 65536)
                    assert t["lds"] == expected_lds(f, t, eb, inverse, n) <= 163840
                    if t["resident"]:
                        assert (t["tile"], t["halo"], t["tiles"]) == (n, 0, 1)
                    else:
                        assert t["tile"] % (1 << levels) == 0 and 0 < t["tile"] <= n
                        assert t["halo"] == halo and t["tiles"] == -(-n // t["tile"])
                        assert inverse or t["tile"] >= min(halo, n)
                        assert t["lds"] <= 98304
            # the depth limit is what pdsp_dwt_max_levels reports on a long row, and every depth on a resident one
            for f in (2, 4, 8, 16, 32):
                most = pdsp.lib.pdsp_dwt_max_levels(f, 1 << 24, eb)
                assert max((f - 2) * ((1 << most) - 1), 1 << most) <= 32768 // eb < max((f - 2) * ((2 << most) - 1), 2 << most)
                assert tile(pdsp, f, most, 1 << 24, eb, False)[0] == 0
                assert tile(pdsp, f, most + 1, 1 << 24, eb, False)[0] == _capi.ERR_UNSUPPORTED_SIZE
                assert pdsp.lib.pdsp_dwt_max_levels(f, 4096, eb) == 12 and pdsp.lib.pdsp_dwt_max_levels(f, 96, eb) == 5
                assert pdsp.lib.pdsp_dwt_max_levels(f, 3 << 20, eb) == min(20, most)
                assert pdsp.lib.pdsp_dwt_max_levels(f, 7, eb) == 0
            assert pdsp.lib.pdsp_dwt_max_levels(3, 64, eb) == 0 and pdsp.lib.pdsp_dwt_max_levels(34, 64, eb) == 0
    assert pdsp.lib.pdsp_dwt_max_levels(4, 64, 2) == 0 and pdsp.lib.pdsp_dwt_max_levels(4, 0, 4) == 0


def test_the_switch_forces_paths_and_caps_tiles(pdsp, tile_switch):
    from pragma_dsp_amd import _capi
    assert tile_switch(2) == 0  # tiled
    for inverse in (False, True):
        rc, t = tile(pdsp, 8, 3, 96, 4, inverse)
        assert rc == 0 and (t["resident"], t["tile"], t["tiles"]) == (0, 96, 1)
        assert t["halo"] == (6 if inverse else 42)
    assert tile_switch(2 | (1 << 2)) == 2  # capped to 2^levels
    rc, t = tile(pdsp, 8, 3, 96, 4, False)
    assert rc == 0 and (t["resident"], t["tile"], t["halo"], t["tiles"]) == (0, 8, 42, 12)
    assert t["lds"] == expected_lds(8, t, 4, False, 96)
    tile_switch(2 | (20 << 2))  # rounded up to a multiple of 2^levels
    assert tile(pdsp, 8, 3, 96, 4, True)[1]["tile"] == 24
    tile_switch(20 << 2)  # a cap alone leaves the choice of path to the rule
    assert tile(pdsp, 8, 3, 96, 4, False)[1]["resident"] == 1
    assert tile(pdsp, 8, 3, 1 << 16, 4, False)[1]["tile"] == 24
    tile_switch(1)  # resident: up to 160 KiB
    rc, t = tile(pdsp, 8, 4, 12288, 4, False)
    assert rc == 0 and t["resident"] == 1 and t["lds"] == 12288 * 6
    rc, _ = tile(pdsp, 8, 4, 1 << 16, 4, False)
    assert rc == _capi.ERR_UNSUPPORTED_SIZE
    assert last(pdsp) == ("the forced resident path has no room for rows of 65536 values of 4 bytes in 160 KiB of LDS "
                          "(pdsp_set_dwt_tile)")
    # a mode that names no path, or a negative one, changes nothing
    assert tile_switch(3) == 1 and tile_switch(-1) == 1 and tile_switch(0) == 1
    for args, text in (((3, 1, 8, 4, 0), "the scaling filter must have an even number of taps, 2 ... 32, got 3"),
                       ((4, 0, 8, 4, 0), "levels must be >= 1, got 0"),
                       ((4, 2, 10, 4, 0), "len must be a positive multiple of 2^levels (levels = 2), got 10"),
                       ((4, 2, 8, 2, 0), "elem_bytes must be 4 or 8, got 2")):
        assert pdsp.lib.pdsp_dev_dwt_tile(*args, (C.c_longlong * 5)()) == _capi.ERR_BAD_ARG and last(pdsp) == text

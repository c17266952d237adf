"""The DCT without a GPU: the f64 numpy restatement of the kernels' maths (Makhoul's algorithm, the norms folded into
two scalars, idct as the dct of the other type) against scipy.fft, which pins the reference the GPU tests use; the
C ABI's argument checks return their status codes and texts before any device work; every new symbol of the header
is in the ctypes table; and the JS declarations of pragma-dsp_amd/js/dct name exactly what dct.js exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "pragma-dsp_amd", "js")
dp = C.POINTER(C.c_double)
vp = C.c_void_p
NORMS = ("backward", "ortho", "forward")
SWAP = {"backward": "forward", "ortho": "ortho", "forward": "backward"}


def dct_scales(n, type, norm):
    """(g, g0): every output (type 2) or input (type 3) times g, index 0 times g0 instead."""
    if norm == "forward":
        return 1.0 / (2 * n), 1.0 / (2 * n)
    if norm == "ortho":
        return 1.0 / np.sqrt(2.0 * n), (1.0 / np.sqrt(4.0 * n) if type == 2 else 1.0 / np.sqrt(n))
    return 1.0, 1.0


def dct_ref(x, type=2, norm="backward"):
    """scipy.fft.dct(x, type, norm) along the last axis in f64, restated as the kernels compute it:
    type 2: v = (x[0::2], x[1::2] reversed), V = rfft(v), y[k] = 2 Re(W_4N^k V[k]), y[N-k] = -2 Im(W_4N^k V[k]);
    type 3: V[k] = conj(W_4N^k) (x[k] - i x[N-k]) / 2 (x[N] = 0), v = irfft(V, N), y[2n] = 2N v[n], y[2n+1] = 2N v[N-1-n]."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1]
    m = n // 2
    g, g0 = dct_scales(n, type, norm)
    k = np.arange(m + 1)
    w4 = np.exp(-1j * np.pi * k / (2 * n))
    if type == 2:
        v = np.concatenate([x[..., 0::2], x[..., 1::2][..., ::-1]], axis=-1)
        c = w4 * np.fft.rfft(v, axis=-1)
        y = np.empty_like(x)
        y[..., :m + 1] = 2 * c.real
        y[..., n - m + 1:] = (-2 * c.imag[..., 1:m])[..., ::-1]
        y *= g
        y[..., 0] *= g0 / g
        return y
    if type == 3:
        xs = x * g
        xs[..., 0] = x[..., 0] * g0
        xr = np.concatenate([np.zeros(x.shape[:-1] + (1,)), xs[..., :0:-1]], axis=-1)  # x[N-k], x[N] = 0
        V = np.conj(w4) * (xs[..., :m + 1] - 1j * xr[..., :m + 1]) / 2
        v = np.fft.irfft(V, n, axis=-1) * (2 * n)
        y = np.empty_like(x)
        y[..., 0::2] = v[..., :m]
        y[..., 1::2] = v[..., m:][..., ::-1]
        return y
    raise ValueError(type)


def idct_ref(x, type=2, norm="backward"):
    return dct_ref(x, 5 - type, SWAP[norm])


@pytest.mark.parametrize("n", [64, 1024, 4096, 16384])
def test_restatement_matches_scipy(n):
    sf = pytest.importorskip("scipy.fft")
    rng = np.random.default_rng(n)
    x = rng.standard_normal((3, n))
    for t in (2, 3):
        for norm in NORMS:
            want = sf.dct(x, type=t, norm=norm, axis=-1)
            got = dct_ref(x, t, norm)
            assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max(), (t, norm)
            want = sf.idct(x, type=t, norm=norm, axis=-1)
            got = idct_ref(x, t, norm)
            assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max(), ("idct", t, norm)


def test_idct_is_the_other_dct_in_scipy():
    sf = pytest.importorskip("scipy.fft")
    x = np.random.default_rng(3).standard_normal(256)
    for t in (2, 3):
        for norm in NORMS:
            assert np.array_equal(sf.idct(x, type=t, norm=norm), sf.dct(x, type=5 - t, norm=SWAP[norm]))


def d(a):
    return a.ctypes.data_as(dp)


def test_dct_host_status_codes_without_device(pdsp):
    from pragma_dsp_amd import _capi
    lib = pdsp.lib
    x, y = np.ones(1 << 15), np.empty(1 << 15)
    cases = [
        ((1, 1000, 2, 0), _capi.ERR_SIZE_NOT_POW2, b"FFT size must be power of two, got 1000"),
        ((1, 0, 2, 0), _capi.ERR_SIZE_NOT_POW2, b"FFT size must be power of two, got 0"),
        ((1, 32, 2, 0), _capi.ERR_UNSUPPORTED_SIZE, b"DCT needs a plan of 64 <= N <= 16384, got 32"),
        ((1, 32768, 2, 0), _capi.ERR_UNSUPPORTED_SIZE, b"DCT needs a plan of 64 <= N <= 16384, got 32768"),
        ((0, 256, 2, 0), _capi.ERR_BAD_ARG, b"batch must be >= 1, got 0"),
        ((-3, 256, 2, 0), _capi.ERR_BAD_ARG, b"batch must be >= 1, got -3"),
        ((1, 256, 1, 0), _capi.ERR_BAD_ARG, b"DCT type must be 2 or 3, got 1"),
        ((1, 256, 4, 0), _capi.ERR_BAD_ARG, b"DCT type must be 2 or 3, got 4"),
        ((1, 256, 2, 3), _capi.ERR_BAD_ARG, b"DCT norm must be 0 (backward), 1 (ortho) or 2 (forward), got 3"),
        ((1, 256, 3, -1), _capi.ERR_BAD_ARG, b"DCT norm must be 0 (backward), 1 (ortho) or 2 (forward), got -1"),
        ((1 << 31, 256, 2, 0), _capi.ERR_BAD_ARG, b"batch 2147483648 x 256 overflows"),
        ((1 << 40, 16384, 2, 0), _capi.ERR_BAD_ARG, b"batch 1099511627776 x 16384 overflows"),
    ]
    for (batch, n, t, norm), code, msg in cases:
        assert lib.pdsp_dct_host_f64(d(x), batch, n, t, norm, d(y)) == code, msg
        assert lib.pdsp_last_error() == msg
    assert lib.pdsp_dct_host_f64(None, 1, 256, 2, 0, d(y)) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"null buffer"
    assert lib.pdsp_dct_host_f64(d(x), 1, 256, 2, 0, None) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"null buffer"


def test_dct_device_entries_refuse_a_null_plan(pdsp):
    from pragma_dsp_amd import _capi
    lib = pdsp.lib
    for fn in (lib.pdsp_dct_f32, lib.pdsp_dct_f64):
        assert fn(None, 1, vp(16), 256, 2, 0, vp(4096), 256, None) == _capi.ERR_BAD_ARG
        assert lib.pdsp_last_error() == b"plan is null"


def test_capi_declares_the_dct_symbols(pdsp):
    from pragma_dsp_amd import _capi
    syms = set(pdsp.lib._pdsp_symbols)
    for name in ("pdsp_dct_f32", "pdsp_dct_f64", "pdsp_dct_host_f64"):
        assert name in syms, name
    assert _capi.DCT_NORMS == {"backward": 0, "ortho": 1, "forward": 2}
    header = open(os.path.join(ROOT, "include", "pdsp_hip.h")).read()
    assert re.search(r"PDSP_DCT_BACKWARD = 0, PDSP_DCT_ORTHO = 1, PDSP_DCT_FORWARD = 2", header)
    for name in ("pdsp_dct_f32", "pdsp_dct_f64", "pdsp_dct_host_f64"):
        assert re.search(r"PDSP_API int %s\(" % name, header), name


def test_python_host_forms_pass_the_errors_through(pdsp):
    from pragma_dsp_amd import PdspError, _capi
    with pytest.raises(PdspError) as e:
        pdsp.dct(np.ones(100))
    assert e.value.code == _capi.ERR_SIZE_NOT_POW2 and str(e.value) == "FFT size must be power of two, got 100"
    with pytest.raises(PdspError) as e:
        pdsp.dct(np.ones(32), type=3)
    assert e.value.code == _capi.ERR_UNSUPPORTED_SIZE and str(e.value) == "DCT needs a plan of 64 <= N <= 16384, got 32"
    with pytest.raises(PdspError) as e:
        pdsp.dct(np.ones(256), type=4)
    assert e.value.code == _capi.ERR_BAD_ARG and str(e.value) == "DCT type must be 2 or 3, got 4"
    with pytest.raises(PdspError) as e:
        pdsp.idct(np.ones(256), type=1)
    assert e.value.code == _capi.ERR_BAD_ARG and str(e.value) == "DCT type must be 2 or 3, got 1"
    with pytest.raises(PdspError) as e:
        pdsp.idct(np.ones(256), norm="unit")
    assert e.value.code == _capi.ERR_BAD_ARG and "DCT norm must be" in str(e.value)
    with pytest.raises(PdspError) as e:
        pdsp.dct(np.ones((2, 2, 64)))
    assert e.value.code == _capi.ERR_BAD_ARG


def _runtime_exports(name):
    src = open(os.path.join(JS, name + ".js")).read()
    body = re.search(r"module\.exports\s*=\s*\{(.*?)\};", src, re.S).group(1)
    return {p.strip().split(":")[0].strip() for p in body.split(",") if p.strip()}


def test_js_declarations_match_dct_exports():
    declared = set(re.findall(r"^export function (\w+)", open(os.path.join(JS, "dct.d.ts")).read(), re.M))
    assert declared == _runtime_exports("dct") == {"dct", "idct"}
    idx = open(os.path.join(JS, "index.d.ts")).read()
    assert re.search(r"export const dct: \{\s*dct: typeof dctNs\.dct;\s*idct: typeof dctNs\.idct;\s*\};", idx)
    js = open(os.path.join(JS, "index.js")).read()
    assert re.search(r"\['dct', \{ dct: dct\.dct, idct: dct\.idct \}\],", js)   # a row of the table of non-enumerable sub-modules
    assert re.search(r"for \(const \[name, value\] of hidden\) Object\.defineProperty\(module\.exports, name, \{ value, "
                     r"enumerable: false \}\);", js)

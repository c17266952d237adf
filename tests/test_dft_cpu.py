"""The any-length DFT (Bluestein's chirp-z algorithm, pdsp_bluestein_kernel.h) without a GPU: the definition the kernel
and its host-built tables implement, restated in numpy and held against numpy.fft.fft; what the C ABI refuses before
any device work; and the bindings' symbol lists.

chirp_z() below is the definition of include/pdsp_hip.h word for word: the chirp c[n] = exp(-i pi (n^2 mod 2L) / L)
with the reduction in integers, M = max(32, the power of two >= 2L - 1), a = x c zero-padded to M, b[j] = conj c[|j|]
at j and M - j, X = c IFFT_M(FFT_M(a) FFT_M(b)).  With a smaller M the circular convolution aliases and the bound
fails (test_a_smaller_m_aliases), which pins the M rule."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "pragma-dsp_amd", "js")

LENGTHS = [2, 3, 5, 16, 17, 32, 33, 97, 255, 257, 1000, 1023, 1025, 2049, 4095, 4096]
SYMBOLS = ("pdsp_dft_create", "pdsp_dft_destroy", "pdsp_dft_length", "pdsp_dft_conv_size", "pdsp_dft_c2c_f32",
           "pdsp_dft_c2c_f64", "pdsp_dft_host_f64")


def conv_size(length):
    """M: the points of the circular convolution."""
    return max(32, 1 << (2 * length - 2).bit_length())


def chirp(length):
    n = np.arange(length, dtype=np.int64)
    return np.exp(-1j * np.pi * ((n * n) % (2 * length)).astype(np.float64) / length)


def chirp_z(x, m=None, inverse=False):
    """The chirp-z DFT of the rows of x in complex128, on transforms of m points (default: the rule)."""
    x = np.asarray(x, np.complex128)
    ln = x.shape[-1]
    m = conv_size(ln) if m is None else m
    c = chirp(ln)
    if inverse:
        x = x.conj()
    a = np.zeros(x.shape[:-1] + (m,), np.complex128)
    a[..., :ln] = x * c
    b = np.zeros(m, np.complex128)
    b[:ln] = c.conj()
    b[m - ln + 1:] = c.conj()[1:][::-1]  # b[M - j] = conj c[j], 0 < j < L
    y = np.fft.ifft(np.fft.fft(a) * np.fft.fft(b))[..., :ln] * c
    return y.conj() / ln if inverse else y


def row_err(got, want):
    """e = max|got - want| / max|want| per row, its maximum over the rows."""
    den = np.abs(want).max(axis=-1, keepdims=True)
    return float((np.abs(got - want) / np.where(den > 0, den, 1.0)).max())


def test_the_m_rule():
    assert [conv_size(n) for n in (2, 16, 17, 32, 33, 64, 65, 1000, 2048, 2049, 4096)] == \
        [32, 32, 64, 64, 128, 128, 256, 2048, 4096, 8192, 8192]
    for ln in range(2, 4097):
        m = conv_size(ln)
        assert m >= 2 * ln - 1 and m >= 32 and (m == 32 or m // 2 < 2 * ln - 1) and m & (m - 1) == 0


@pytest.mark.parametrize("ln", LENGTHS)
def test_restatement_against_numpy(ln):
    rng = np.random.default_rng(ln)
    x = rng.standard_normal((3, ln)) + 1j * rng.standard_normal((3, ln))
    assert row_err(chirp_z(x), np.fft.fft(x)) <= 1e-12
    assert row_err(chirp_z(x, inverse=True), np.fft.ifft(x)) <= 1e-12
    assert row_err(chirp_z(x.real), np.fft.fft(x.real)) <= 1e-12


@pytest.mark.parametrize("ln", [18, 35, 97, 1000, 4095])
def test_a_smaller_m_aliases(ln):
    # (L = 2^k + 1 is left out: there M / 2 = 2L - 2, and the one lag that wraps, -(L - 1) onto L - 1, meets its own
    # value, b being even)
    rng = np.random.default_rng(ln)
    x = rng.standard_normal((3, ln)) + 1j * rng.standard_normal((3, ln))
    assert row_err(chirp_z(x, m=conv_size(ln) // 2), np.fft.fft(x)) > 1e-3


def test_create_refuses_unsupported_lengths_and_leaves_out_untouched(pdsp):
    from pragma_dsp_amd import _capi
    lib = pdsp.lib
    for ln in (1, 0, -3, 4097):
        h = C.c_void_p(0x1234)
        assert lib.pdsp_dft_create(ln, -1, C.byref(h)) == _capi.ERR_UNSUPPORTED_SIZE
        assert lib.pdsp_last_error() == b"DFT length must be 2 ... 4096, got %d" % ln
        assert h.value == 0x1234
    assert lib.pdsp_dft_create(1000, -1, None) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"out is null"
    for fn in (pdsp.dft, pdsp.idft):
        for ln in (1, 4097):
            with pytest.raises(pdsp.PdspError) as e:
                fn(np.ones(ln))
            assert e.value.code == _capi.ERR_UNSUPPORTED_SIZE and str(e.value) == f"DFT length must be 2 ... 4096, got {ln}"
    with pytest.raises(pdsp.PdspError) as e:
        pdsp.Dft(4097)
    assert e.value.code == _capi.ERR_UNSUPPORTED_SIZE
    with pytest.raises(pdsp.PdspError) as e:
        pdsp.Dft(2.5)
    assert e.value.code == _capi.ERR_BAD_ARG


def test_null_handles_are_refused_before_any_device_work(pdsp):
    from pragma_dsp_amd import _capi
    lib = pdsp.lib
    vp = C.c_void_p
    for fn in (lib.pdsp_dft_c2c_f32, lib.pdsp_dft_c2c_f64):
        for inverse in (0, 1):
            assert fn(None, 1, vp(16), vp(32), 8, vp(64), vp(128), 8, inverse, None) == _capi.ERR_BAD_ARG
            assert lib.pdsp_last_error() == b"dft is null"
    assert lib.pdsp_dft_destroy(None) == 0
    assert lib.pdsp_dft_length(None) == 0 and lib.pdsp_dft_conv_size(None) == 0
    x = np.ones(8)
    assert lib.pdsp_dft_host_f64(None, None, 1, 8, 0, _capi.dptr(x), _capi.dptr(x)) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"null buffer"
    assert lib.pdsp_dft_host_f64(_capi.dptr(x), None, 0, 8, 0, _capi.dptr(x), _capi.dptr(x)) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"batch must be >= 1, got 0"


def test_capi_declares_the_dft_symbols(pdsp):
    syms = set(pdsp.lib._pdsp_symbols)
    header = open(os.path.join(ROOT, "include", "pdsp_hip.h")).read()
    declared = set(re.findall(r"PDSP_API\s+[\w\s\*]+?\b(pdsp_dft_\w+)\s*\(", header))
    assert declared == set(SYMBOLS)
    for name in SYMBOLS:
        assert name in syms, name
    assert "typedef struct pdsp_dft pdsp_dft;" in header
    for name in ("Dft", "dft", "idft"):
        assert name in pdsp.__all__ and callable(getattr(pdsp, name))
    assert callable(pdsp.Dft.forward) and callable(pdsp.Dft.inverse)


def _runtime_exports(name):
    src = open(os.path.join(JS, name + ".js")).read()
    body = re.search(r"module\.exports\s*=\s*\{(.*?)\};", src, re.S).group(1)
    return {p.strip().split(":")[0].strip() for p in body.split(",") if p.strip()}


def test_js_declarations_match_dft_exports():
    declared = set(re.findall(r"^export function (\w+)", open(os.path.join(JS, "dft.d.ts")).read(), re.M))
    assert declared == _runtime_exports("dft") == {"dft", "idft"}
    idx = open(os.path.join(JS, "index.d.ts")).read()
    assert re.search(r"export const dft: \{\s*dft: typeof dftNs\.dft;\s*idft: typeof dftNs\.idft;\s*\};", idx)
    js = open(os.path.join(JS, "index.js")).read()
    assert re.search(r"\['dft', \{ dft: dft\.dft, idft: dft\.idft \}\],", js)   # a row of the table of non-enumerable sub-modules
    assert re.search(r"for \(const \[name, value\] of hidden\) Object\.defineProperty\(module\.exports, name, \{ value, "
                     r"enumerable: false \}\);", js)
    napi = open(os.path.join(ROOT, "pragma-dsp_amd", "csrc", "pdsp_napi.c")).read()
    assert napi.count("pdsp_dft_") == 1 and '{"dft", Dft}' in napi  # one binding, of the host form

"""The Hilbert transform without a GPU: the f64 numpy restatement of the definition the kernel implements (rfft, -i on
the positive-frequency bins, zeros at DC and Nyquist, irfft) against scipy.signal.hilbert, which pins the reference the
GPU tests use, and its known answers; the C ABI's argument checks return their status codes and texts before any
device work; every new symbol of the header is in the ctypes table; and the JS declarations of
pragma-dsp_amd/js/hilbert name exactly what hilbert.js exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "pragma-dsp_amd", "js")
dp = C.POINTER(C.c_double)
vp = C.c_void_p
NS = [64 << i for i in range(9)]  # 64 ... 16384
MODES = ("analytic", "imag", "envelope", "phase")


def hilbert_ref(x, n=None):
    """scipy.signal.hilbert(x, N=n) along the last axis in f64 (n even, n >= len), as the kernel computes it:
    X = rfft(x zero-padded to n), Y[k] = -i X[k] for 0 < k < n/2, Y[0] = Y[n/2] = 0, Hx = irfft(Y, n); x + i Hx."""
    x = np.asarray(x, dtype=np.float64)
    ln = x.shape[-1]
    n = ln if n is None else n
    assert n % 2 == 0 and n >= ln
    xp = np.zeros(x.shape[:-1] + (n,))
    xp[..., :ln] = x
    y = -1j * np.fft.rfft(xp, axis=-1)
    y[..., 0] = 0
    y[..., n // 2] = 0
    return xp + 1j * np.fft.irfft(y, n, axis=-1)


def mode_ref(a, mode):
    """What each output mode is of the analytic signal a."""
    return {"analytic": a, "imag": a.imag, "envelope": np.abs(a), "phase": np.angle(a)}[mode]


@pytest.mark.parametrize("n", NS)
def test_restatement_matches_scipy(n):
    ss = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(n)
    x = rng.standard_normal((3, n))
    want = ss.hilbert(x, axis=-1)
    assert np.abs(hilbert_ref(x) - want).max() <= 1e-13
    for ln in (1, n // 2, n - 1):  # zero padding: scipy's N
        want = ss.hilbert(x[:, :ln], N=n, axis=-1)
        assert np.abs(hilbert_ref(x[:, :ln], n) - want).max() <= 1e-13, ln


@pytest.mark.parametrize("n", [64, 1024, 16384])
def test_restatement_known_answers(n):
    nn = np.arange(n)
    for k in (1, 5, n // 4, n // 2 - 1):
        # the angle reduced exactly (integer phase mod n) so that the inputs are correct to the last bit
        ph = 2 * np.pi * ((k * nn) % n) / n
        a = hilbert_ref(np.cos(ph))
        assert np.abs(a.imag - np.sin(ph)).max() <= 1e-13, k
        assert np.abs(np.abs(a) - 1).max() <= 1e-13, k
    assert np.array_equal(hilbert_ref(np.full(n, 0.75)).imag, np.zeros(n))
    assert np.array_equal(hilbert_ref((-1.0) ** nn).imag, np.zeros(n))
    a = hilbert_ref(np.ones(3), n)
    assert np.array_equal(a.real, np.r_[np.ones(3), np.zeros(n - 3)])


def d(a):
    return a.ctypes.data_as(dp)


def test_hilbert_host_status_codes_without_device(pdsp):
    from pragma_dsp_amd import _capi
    lib = pdsp.lib
    x, y = np.ones(1 << 15), np.empty(1 << 16)
    cases = [
        ((1, 1000, 1000, 0), _capi.ERR_SIZE_NOT_POW2, b"FFT size must be power of two, got 1000"),
        ((1, 1, 0, 1), _capi.ERR_SIZE_NOT_POW2, b"FFT size must be power of two, got 0"),
        ((1, 32, 32, 1), _capi.ERR_UNSUPPORTED_SIZE, b"the Hilbert transform needs a plan of 64 <= N <= 16384, got 32"),
        ((1, 100, 32768, 2), _capi.ERR_UNSUPPORTED_SIZE,
         b"the Hilbert transform needs a plan of 64 <= N <= 16384, got 32768"),
        ((0, 256, 256, 0), _capi.ERR_BAD_ARG, b"batch must be >= 1, got 0"),
        ((-3, 256, 256, 0), _capi.ERR_BAD_ARG, b"batch must be >= 1, got -3"),
        ((1, 0, 256, 0), _capi.ERR_BAD_ARG, b"len must be 1 ... N = 256, got 0"),
        ((1, 257, 256, 3), _capi.ERR_BAD_ARG, b"len must be 1 ... N = 256, got 257"),
        ((1, 256, 256, 4), _capi.ERR_BAD_ARG,
         b"Hilbert output must be 0 (analytic), 1 (imag), 2 (envelope) or 3 (phase), got 4"),
        ((1, 256, 256, -1), _capi.ERR_BAD_ARG,
         b"Hilbert output must be 0 (analytic), 1 (imag), 2 (envelope) or 3 (phase), got -1"),
        ((1 << 31, 256, 256, 1), _capi.ERR_BAD_ARG, b"batch 2147483648 x 256 overflows"),
        ((1 << 40, 16384, 16384, 0), _capi.ERR_BAD_ARG, b"batch 1099511627776 x 16384 overflows"),
    ]
    for (batch, ln, n, mode), code, msg in cases:
        assert lib.pdsp_hilbert_host_f64(d(x), batch, ln, n, mode, d(y)) == code, msg
        assert lib.pdsp_last_error() == msg
    assert lib.pdsp_hilbert_host_f64(None, 1, 256, 256, 0, d(y)) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"null buffer"
    assert lib.pdsp_hilbert_host_f64(d(x), 1, 256, 256, 2, None) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"null buffer"


def test_hilbert_device_entries_refuse_a_null_plan(pdsp):
    from pragma_dsp_amd import _capi
    lib = pdsp.lib
    for fn in (lib.pdsp_hilbert_f32, lib.pdsp_hilbert_f64):
        for mode in range(4):
            assert fn(None, 1, vp(16), 256, 256, mode, vp(4096), 512, None) == _capi.ERR_BAD_ARG
            assert lib.pdsp_last_error() == b"plan is null"


def test_capi_declares_the_hilbert_symbols(pdsp):
    from pragma_dsp_amd import _capi
    syms = set(pdsp.lib._pdsp_symbols)
    names = ("pdsp_hilbert_f32", "pdsp_hilbert_f64", "pdsp_hilbert_host_f64")
    for name in names:
        assert name in syms, name
    assert _capi.HILBERT_OUT == {"analytic": 0, "imag": 1, "envelope": 2, "phase": 3}
    header = open(os.path.join(ROOT, "include", "pdsp_hip.h")).read()
    assert re.search(r"PDSP_HILBERT_ANALYTIC = 0,\s*PDSP_HILBERT_IMAG = 1,\s*PDSP_HILBERT_ENVELOPE = 2,\s*"
                     r"PDSP_HILBERT_PHASE = 3", header)
    for name in names:
        assert re.search(r"PDSP_API int %s\(" % name, header), name
    for name in ("hilbert", "envelope", "instantaneous_phase"):
        assert name in pdsp.__all__ and callable(getattr(pdsp, name))
    from pragma_dsp_amd.batch import BatchedFft
    for name in ("hilbert", "hilbert_imag", "envelope", "instantaneous_phase"):
        assert callable(getattr(BatchedFft, name))


def test_python_host_forms_pass_the_errors_through(pdsp):
    from pragma_dsp_amd import PdspError, _capi
    for fn in (pdsp.hilbert, pdsp.envelope, pdsp.instantaneous_phase):
        with pytest.raises(PdspError) as e:
            fn(np.ones(100))
        assert e.value.code == _capi.ERR_SIZE_NOT_POW2 and str(e.value) == "FFT size must be power of two, got 100"
        with pytest.raises(PdspError) as e:
            fn(np.ones(32))
        assert e.value.code == _capi.ERR_UNSUPPORTED_SIZE
        assert str(e.value) == "the Hilbert transform needs a plan of 64 <= N <= 16384, got 32"
        with pytest.raises(PdspError) as e:
            fn(np.ones(100), n=32768)
        assert e.value.code == _capi.ERR_UNSUPPORTED_SIZE
        with pytest.raises(PdspError) as e:
            fn(np.ones(300), n=256)  # truncation is the caller's slice
        assert e.value.code == _capi.ERR_BAD_ARG and str(e.value) == "len must be 1 ... N = 256, got 300"
        with pytest.raises(PdspError) as e:
            fn(np.ones((2, 2, 64)))
        assert e.value.code == _capi.ERR_BAD_ARG
        with pytest.raises(PdspError) as e:
            fn(np.ones((2, 0)), n=64)
        assert e.value.code == _capi.ERR_BAD_ARG


def _runtime_exports(name):
    src = open(os.path.join(JS, name + ".js")).read()
    body = re.search(r"module\.exports\s*=\s*\{(.*?)\};", src, re.S).group(1)
    return {p.strip().split(":")[0].strip() for p in body.split(",") if p.strip()}


def test_js_declarations_match_hilbert_exports():
    declared = set(re.findall(r"^export function (\w+)", open(os.path.join(JS, "hilbert.d.ts")).read(), re.M))
    assert declared == _runtime_exports("hilbert") == {"hilbert", "envelope", "instantaneousPhase"}
    idx = open(os.path.join(JS, "index.d.ts")).read()
    assert re.search(r"export const hilbert: \{\s*hilbert: typeof hilbertNs\.hilbert;\s*envelope: typeof "
                     r"hilbertNs\.envelope;\s*instantaneousPhase: typeof hilbertNs\.instantaneousPhase;\s*\};", idx)
    js = open(os.path.join(JS, "index.js")).read()
    assert re.search(r"\['hilbert', \{ hilbert: hilbert\.hilbert, envelope: hilbert\.envelope, instantaneousPhase: "
                     r"hilbert\.instantaneousPhase \}\],", js)   # a row of the table of non-enumerable sub-modules
    assert re.search(r"for \(const \[name, value\] of hidden\) Object\.defineProperty\(module\.exports, name, \{ value, "
                     r"enumerable: false \}\);", js)

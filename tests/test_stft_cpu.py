"""The short-time pair without a GPU: the C ABI's argument checks return their status codes and texts before any
device work, every new symbol of the header is in the ctypes table, the Python host forms pass the same errors
through, and the JS declarations of pragma-dsp_amd/js/stft name exactly what stft.js exports."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "pragma-dsp_amd", "js")
dp = C.POINTER(C.c_double)
vp = C.c_void_p


def d(a):
    return a.ctypes.data_as(dp)


def test_stft_host_status_codes_without_device(pdsp):
    from pragma_dsp_amd import _capi
    lib = pdsp.lib
    x, re_, im_ = np.ones(4096), np.empty(1 << 16), np.empty(1 << 16)
    cases = [
        ((d(x), 4096, 1000, 64, 1), _capi.ERR_SIZE_NOT_POW2, b"FFT size must be power of two, got 1000"),
        ((d(x), 4096, 32, 8, 1), _capi.ERR_UNSUPPORTED_SIZE, b"STFT needs a plan of 64 <= N <= 16384, got 32"),
        ((d(x), 4096, 32768, 8, 1), _capi.ERR_UNSUPPORTED_SIZE, b"STFT needs a plan of 64 <= N <= 16384, got 32768"),
        ((d(x), 4096, 256, 0, 1), _capi.ERR_BAD_ARG, b"hop must be >= 1, got 0"),
        ((d(x), 4096, 256, -5, 1), _capi.ERR_BAD_ARG, b"hop must be >= 1, got -5"),
        ((d(x), 4096, 256, 64, 9), _capi.ERR_WINDOW_TYPE, b"Unsupported window type: 9"),
        ((d(x), 100, 256, 64, 1), _capi.ERR_INPUT_LENGTH, b"signal length 100 is shorter than one frame (256)"),
        ((d(x), 1 << 50, 256, 1, 1), _capi.ERR_BAD_ARG, b"signal too long: 1125899906842624 samples"),
        ((None, 4096, 256, 64, 1), _capi.ERR_BAD_ARG, b"null buffer"),
    ]
    for (sig, length, n, hop, win), code, msg in cases:
        assert lib.pdsp_stft_host_f64(sig, length, n, hop, win, d(re_), d(im_)) == code, msg
        assert lib.pdsp_last_error() == msg
    icases = [
        ((2, 1000, 64, 1), _capi.ERR_SIZE_NOT_POW2, b"FFT size must be power of two, got 1000"),
        ((2, 16, 8, 1), _capi.ERR_UNSUPPORTED_SIZE, b"STFT needs a plan of 64 <= N <= 16384, got 16"),
        ((2, 256, 0, 1), _capi.ERR_BAD_ARG, b"hop must be >= 1, got 0"),
        ((2, 256, 64, -1), _capi.ERR_WINDOW_TYPE, b"Unsupported window type: -1"),
        ((0, 256, 64, 1), _capi.ERR_BAD_ARG, b"frames must be >= 1, got 0"),
        ((1 << 40, 256, 1 << 40, 1), _capi.ERR_BAD_ARG, b"frames 1099511627776 x hop 1099511627776 overflows"),
        ((3, 256, (1 << 62), 1), _capi.ERR_BAD_ARG, b"frames 3 x hop 4611686018427387904 overflows"),
    ]
    out = np.empty(1 << 16)
    for (frames, n, hop, win), code, msg in icases:
        assert lib.pdsp_istft_host_f64(d(re_), d(im_), frames, n, hop, win, d(out)) == code, msg
        assert lib.pdsp_last_error() == msg
    assert lib.pdsp_istft_host_f64(None, d(im_), 2, 256, 64, 1, d(out)) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"null buffer"


def test_stft_device_entries_check_the_plan_first(pdsp):
    from pragma_dsp_amd import _capi
    lib = pdsp.lib
    for sfx in ("f32", "f64"):
        assert getattr(lib, "pdsp_stft_complex_" + sfx)(None, 4, vp(0), 256, 64, vp(0), vp(0), vp(0), vp(0)) == _capi.ERR_BAD_ARG
        assert lib.pdsp_last_error() == b"plan is null"
        assert getattr(lib, "pdsp_istft_" + sfx)(None, 4, vp(0), vp(0), 64, vp(0), vp(0), vp(0)) == _capi.ERR_BAD_ARG
        assert lib.pdsp_last_error() == b"plan is null"


def test_istft_chunk_switch_returns_previous_value(pdsp):
    lib = pdsp.lib
    prev = lib.pdsp_set_istft_chunk_frames(7)
    try:
        assert lib.pdsp_set_istft_chunk_frames(-3) == 7
        assert lib.pdsp_set_istft_chunk_frames(0) == 0  # a negative value means the default (0)
    finally:
        lib.pdsp_set_istft_chunk_frames(prev)


def test_python_host_forms_raise_the_library_errors(pdsp):
    from pragma_dsp_amd import _capi
    from pragma_dsp_amd._capi import PdspError
    x = np.zeros(1000)
    for call, code, text in (
        (lambda: pdsp.stft(x, 256, 0), _capi.ERR_BAD_ARG, "hop must be >= 1, got 0"),
        (lambda: pdsp.stft(x[:100], 256, 64), _capi.ERR_INPUT_LENGTH, "signal length 100 is shorter than one frame (256)"),
        (lambda: pdsp.stft(x, 1 << 40, 64), _capi.ERR_UNSUPPORTED_SIZE, "STFT needs a plan of 64 <= N <= 16384"),
        (lambda: pdsp.stft(x, 255, 64), _capi.ERR_SIZE_NOT_POW2, "FFT size must be power of two, got 255"),
        (lambda: pdsp.stft(x, 256, 64, "kaiser"), _capi.ERR_WINDOW_TYPE, "Unsupported window type: kaiser"),
        (lambda: pdsp.stft(np.zeros((4, 300)), 256, 64), _capi.ERR_BAD_ARG, "signal must be 1-D"),
        (lambda: pdsp.istft(np.zeros((2, 129), complex), 0), _capi.ERR_BAD_ARG, "hop must be >= 1, got 0"),
        (lambda: pdsp.istft(np.zeros((2, 17), complex), 4), _capi.ERR_UNSUPPORTED_SIZE, "got 32"),
        (lambda: pdsp.istft(np.zeros((2, 129), complex), 1 << 45), _capi.ERR_BAD_ARG, "overflows"),
        (lambda: pdsp.istft(np.zeros(129, complex), 64), _capi.ERR_BAD_ARG, "spec must be"),
    ):
        with pytest.raises(PdspError) as e:
            call()
        assert e.value.code == code and text in str(e.value), (str(e.value), text)
    assert "stft" in pdsp.__all__ and "istft" in pdsp.__all__


def test_every_stft_symbol_is_bound(pdsp):
    hdr = open(os.path.join(ROOT, "include", "pdsp_hip.h")).read() + open(os.path.join(ROOT, "include", "pdsp_hip_dev.h")).read()
    names = set(re.findall(r"PDSP_API int (pdsp_(?:stft|istft|set_istft)\w*)\(", hdr))
    assert names == {"pdsp_stft_complex_f32", "pdsp_stft_complex_f64", "pdsp_istft_f32", "pdsp_istft_f64",
                     "pdsp_stft_host_f64", "pdsp_istft_host_f64", "pdsp_set_istft_chunk_frames"}
    assert names <= set(pdsp.lib._pdsp_symbols)


def _runtime_exports(name):
    src = open(os.path.join(JS, name + ".js")).read()
    body = re.search(r"module\.exports\s*=\s*\{(.*?)\};", src, re.S).group(1)
    return {p.strip().split(":")[0] for p in body.split(",") if p.strip()}


def test_stft_declarations_match_runtime_exports():
    decl = set(re.findall(r"^export (?:declare )?(?:function|class|const) (\w+)", open(os.path.join(JS, "stft.d.ts")).read(), re.M))
    assert decl == _runtime_exports("stft") == {"stft", "istft"}
    idx = open(os.path.join(JS, "index.d.ts")).read()
    assert re.search(r"export const stft: \{\s*stft: typeof stftNs\.stft;\s*istft: typeof stftNs\.istft;\s*\};", idx)


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists(os.path.join(ROOT, "pragma-dsp_amd", "csrc", "pdsp_napi.node")),
                    reason="node or the addon is not available")
def test_js_stft_is_hidden_and_checks_before_the_device():
    script = r"""
const p = require(process.argv[1]);
const out = {keys: Object.keys(p), hidden: Object.keys(p.stft)};
const errs = [];
for (const f of [
  () => p.stft.stft([1, 2, 3], {fftSize: 64, hopSize: 1}),
  () => p.stft.stft(new Float32Array(100), {fftSize: 32, hopSize: 1}),
  () => p.stft.stft('abc', {fftSize: 64, hopSize: 1}),
  () => p.stft.stft([], {fftSize: 64, hopSize: 1, window: 'kaiser'}),
  () => p.stft.stft(new Array(100).fill(0), {fftSize: 64, hopSize: 0}),
  () => p.stft.stft(new Array(100).fill(0), {fftSize: 2 ** 40, hopSize: 1}),
  () => p.stft.istft({frames: 1, real: [1], imag: [1]}, {fftSize: 64, hopSize: 1}),
  () => p.stft.istft({frames: 0, real: [], imag: []}, {fftSize: 64, hopSize: 1}),
  () => p.stft.istft({frames: 2, real: new Float64Array(66), imag: new Float64Array(66)}, {fftSize: 64, hopSize: 2 ** 52}),
]) { try { f(); errs.push(null); } catch (e) { errs.push(e.message); } }
out.errs = errs;
console.log(JSON.stringify(out));
"""
    import json
    res = subprocess.run(["node", "-e", script, os.path.join(JS)], capture_output=True, text=True, timeout=60, check=True)
    got = json.loads(res.stdout)
    assert got["keys"] == ["spectrum", "spectrumBatch", "spectrumStream", "core", "fourier"]
    assert got["hidden"] == ["stft", "istft"]
    assert got["errs"] == [
        "signal length 3 is shorter than one frame (64)",
        "STFT needs a plan of 64 <= N <= 16384, got 32",
        "signal must be an array or a typed array",
        "Unsupported window type: kaiser",
        "hop must be >= 1, got 0",
        "STFT needs a plan of 64 <= N <= 16384, got 1099511627776",
        "real and imag must hold frames * (fftSize/2 + 1) = 33 values, got 1 and 1",
        "frames must be an integer >= 1, got 0",
        "frames 2 x hop 4503599627370496 overflows",
    ]

"""FIR filtering without a GPU: the C ABI's argument checks return their status codes and texts before any device
work, every FIR symbol of the header is in the ctypes table, the mode ranges follow numpy.convolve, and the JS
declarations of pragma-dsp_amd/js/filters name exactly what filters.js exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JS = os.path.join(ROOT, "pragma-dsp_amd", "js")
dp = C.POINTER(C.c_double)


def d(a):
    return a.ctypes.data_as(dp)


def test_fir_status_codes_without_device(pdsp):
    from pragma_dsp_amd import _capi
    lib = pdsp.lib
    x, h, y = np.ones(16), np.ones(4), np.empty(64)
    assert lib.pdsp_fir_filter_host_f64(d(x), 1, 16, d(h), 0, 0, d(y)) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"filter must have at least one tap, got 0"
    assert lib.pdsp_fir_filter_host_f64(d(x), 1, 16, d(h), 8193, 0, d(y)) == _capi.ERR_UNSUPPORTED_SIZE
    assert b"exceeds N/2 = 8192" in lib.pdsp_last_error()
    assert lib.pdsp_fir_filter_host_f64(d(x), -1, 16, d(h), 4, 0, d(y)) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"batch must be >= 0, got -1"
    assert lib.pdsp_fir_filter_host_f64(d(x), 1, -3, d(h), 4, 0, d(y)) == _capi.ERR_BAD_ARG
    assert lib.pdsp_fir_filter_host_f64(d(x), 1, 16, d(h), 4, 7, d(y)) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"unknown FIR mode 7"
    assert lib.pdsp_fir_filter_host_f64(d(x), 1 << 40, 1 << 30, d(h), 4, 0, d(y)) == _capi.ERR_BAD_ARG
    assert b"overflows" in lib.pdsp_last_error()
    # the device entries check their plan first (no plan exists without a GPU)
    vp = C.c_void_p
    assert lib.pdsp_fir_filter_f32(None, 1, vp(0), 16, 16, vp(0), vp(0), 4, 0, 19, vp(0), 19, vp(0)) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"plan is null"
    assert lib.pdsp_fir_spectrum_f64(None, vp(0), 4, vp(0), vp(0), vp(0)) == _capi.ERR_BAD_ARG
    assert lib.pdsp_fir_block_size(0) == 0 and lib.pdsp_fir_block_size(8193) == 0
    assert [lib.pdsp_fir_block_size(p) for p in (1, 512, 513, 1024, 2048, 2049, 8192)] == \
        [4096, 4096, 8192, 8192, 16384, 16384, 16384]
    if lib.pdsp_device_count() == 0:
        assert lib.pdsp_fir_filter_host_f64(d(x), 1, 16, d(h), 4, 0, d(y)) == _capi.ERR_DEVICE
        with pytest.raises(pdsp.PdspError, match="no HIP device"):
            pdsp.firFilter(x, h)


@pytest.mark.parametrize("n,p", [(10, 3), (3, 10), (7, 7), (1, 1), (8, 1), (1, 5), (6, 4), (4, 6)])
def test_mode_ranges_follow_numpy_convolve(pdsp, n, p):
    from pragma_dsp_amd.filters import output_range
    rng = np.random.default_rng(n * 31 + p)
    x, h = rng.standard_normal(n), rng.standard_normal(p)
    full = np.convolve(x, h)
    for mode in ("full", "same", "valid"):
        off, ln = output_range(n, p, mode)
        assert np.array_equal(full[off:off + ln], np.convolve(x, h, mode=mode)), mode
    assert output_range(n, p, "filter") == (0, n)
    with pytest.raises(pdsp.PdspError, match="unknown FIR mode"):
        output_range(n, p, "circular")


def test_fir_symbols_in_ctypes_table(pdsp):
    hdr = open(os.path.join(ROOT, "include", "pdsp_hip.h")).read()
    fir = set(re.findall(r"PDSP_API\s+[\w\s\*]+?\b(pdsp_fir_\w+)\s*\(", hdr))
    assert fir == {"pdsp_fir_spectrum_f32", "pdsp_fir_spectrum_f64", "pdsp_fir_filter_f32", "pdsp_fir_filter_f64",
                   "pdsp_fir_output_range", "pdsp_fir_block_size", "pdsp_fir_filter_host_f64"}
    assert fir <= set(pdsp.lib._pdsp_symbols)
    for name in ("FirFilter", "fir_filter", "firFilter"):
        assert name in pdsp.__all__ and callable(getattr(pdsp, name))


def test_js_filters_declarations_match_exports():
    src = open(os.path.join(JS, "filters.js")).read()
    body = re.search(r"module\.exports\s*=\s*\{(.*?)\};", src, re.S).group(1)
    runtime = {p.strip().split(":")[0] for p in body.split(",") if p.strip()}
    decl = set(re.findall(r"^export (?:declare )?(?:function|class|const) (\w+)", open(os.path.join(JS, "filters.d.ts")).read(),
                          re.M))
    assert decl == runtime == {"firFilter"}
    idx_js = open(os.path.join(JS, "index.js")).read()
    idx_ts = open(os.path.join(JS, "index.d.ts")).read()
    assert re.search(r"'filters'", idx_js) and re.search(r"export const filters\b", idx_ts)
    assert re.search(r"firFilter: typeof filtersNs\.firFilter", idx_ts)

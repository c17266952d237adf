"""pdsp_dev_transform_path_* / pdsp_dev_spectrum_path_* without a device: the argument checks they share with the calls
they describe come first, so a null plan is refused with the call's own code and text -- with or without an info
array -- and nothing is written.  What they report for a real plan is tests/test_gpu_dispatch_queries.py."""
import ctypes as C

PDSP_ERR_BAD_ARG = 9
PATH_INFO = 17  # PDSP_DEV_PATH_INFO


def _queries(lib):
    t = lambda fn: (lambda info: fn(None, 2, None, None, None, None, 0, info))  # noqa: E731
    s = lambda fn: (lambda info: fn(None, 2, None, 64, 64, None, 0, None, None, None, None, 1.0, info))  # noqa: E731
    return {"pdsp_dev_transform_path_f32": t(lib.pdsp_dev_transform_path_f32),
            "pdsp_dev_transform_path_f64": t(lib.pdsp_dev_transform_path_f64),
            "pdsp_dev_spectrum_path_f32": s(lib.pdsp_dev_spectrum_path_f32),
            "pdsp_dev_spectrum_path_f64": s(lib.pdsp_dev_spectrum_path_f64)}


def test_null_plan_is_refused_like_the_call(pdsp):
    lib = pdsp.lib
    # the text the calls themselves give for a null plan
    assert lib.pdsp_fft_forward_real_f32(None, 2, None, None, None, None) == PDSP_ERR_BAD_ARG
    want = lib.pdsp_last_error()
    assert want == b"plan is null"
    amp = (C.c_double * 4)()  # pdsp_spectrum_* looks at amp_out before the plan; never written: the plan is null
    assert lib.pdsp_spectrum_f64(None, 2, None, 64, 64, None, 0, C.addressof(amp), None, None, None) == PDSP_ERR_BAD_ARG
    assert lib.pdsp_last_error() == want
    for name, q in _queries(lib).items():
        info = (C.c_int * PATH_INFO)(*([-7] * PATH_INFO))
        assert q(info) == PDSP_ERR_BAD_ARG, name
        assert lib.pdsp_last_error() == want, name
        assert list(info) == [-7] * PATH_INFO, name
        assert q(None) == PDSP_ERR_BAD_ARG, name
        assert lib.pdsp_last_error() == want, name
    # the inverse's entry point checks the plan itself, before it exchanges the planes
    for fn in (lib.pdsp_dev_transform_path_f32, lib.pdsp_dev_transform_path_f64):
        assert fn(None, 2, None, None, None, None, 1, None) == PDSP_ERR_BAD_ARG
        assert lib.pdsp_last_error() == want


def test_header_and_ctypes_symbols_agree(pdsp):
    from test_capi_cpu import header_symbols
    dev = header_symbols("pdsp_hip_dev.h")
    assert sorted(dev) == sorted([
        "pdsp_set_split16k", "pdsp_set_staged_small", "pdsp_set_fused_window", "pdsp_set_twopass",
        "pdsp_set_real_packed", "pdsp_set_istft_chunk_frames", "pdsp_set_upfirdn_tile", "pdsp_dev_upfirdn_tile",
        "pdsp_set_dwt_tile", "pdsp_dev_dwt_tile", "pdsp_dev_complex_op_vec4", "pdsp_dev_transform_path_f32",
        "pdsp_dev_transform_path_f64", "pdsp_dev_spectrum_path_f32", "pdsp_dev_spectrum_path_f64",
        "pdsp_dev_host_transform_chunks", "pdsp_dev_host_spectrum_chunks", "pdsp_dev_live_resources"])
    assert not [s for s in header_symbols() if "_path_" in s]
    raw = C.CDLL(pdsp.LIB_PATH)
    for s in dev:
        assert s in pdsp.lib._pdsp_symbols and hasattr(raw, s), s
    import os
    import re
    from test_capi_cpu import ROOT
    text = open(os.path.join(ROOT, "include", "pdsp_hip_dev.h")).read()
    assert re.findall(r"#define\s+PDSP_DEV_PATH_INFO\s+(\d+)", text) == [str(PATH_INFO)]

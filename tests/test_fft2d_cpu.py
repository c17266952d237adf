"""The 2-D transform's boundary without a GPU: include/pdsp_hip_fft2d.h against the library and the ctypes binding, the
refusals that come ahead of the device check, and pdsp_fft2d_query over the whole domain and its edges against the
rule written out here."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pdsp_hip_fft2d.h")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SYMBOLS = ["pdsp_fft2d_c2c_f32", "pdsp_fft2d_c2c_f64", "pdsp_fft2d_create", "pdsp_fft2d_destroy", "pdsp_fft2d_height",
           "pdsp_fft2d_host_f64", "pdsp_fft2d_query", "pdsp_fft2d_width"]
ERR_UNSUPPORTED_SIZE, ERR_BAD_ARG = 8, 9


def header_symbols(path):
    return sorted(set(re.findall(r"PDSP_API\s+[\w\s\*]+?\b(pdsp_\w+)\s*\(", open(path).read())))


def test_every_symbol_of_the_header_is_exported_and_bound(pdsp):
    assert header_symbols(HEADER) == SYMBOLS
    raw = C.CDLL(pdsp.LIB_PATH)
    for s in SYMBOLS:
        assert hasattr(raw, s), f"{s} declared in include/pdsp_hip_fft2d.h but not exported"
        assert getattr(pdsp.lib, s).argtypes is not None, s
    assert sorted(pdsp.lib._pdsp_fft2d_symbols) == SYMBOLS
    # the two older headers and their table are as they were: no name of this family in them, none claims pdsp_fft_
    assert not set(SYMBOLS) & set(pdsp.lib._pdsp_symbols)
    assert not [s for s in SYMBOLS if s.startswith("pdsp_fft_")]
    for h in ("pdsp_hip.h", "pdsp_hip_dev.h"):
        text = open(os.path.join(ROOT, "include", h)).read()
        assert "fft2d" not in text, h


def test_header_is_valid_c11_and_declares_the_enums(tmp_path):
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    inc = "-I" + os.path.join(ROOT, "include")
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", inc, "-fsyntax-only", "-x", "c", HEADER],
                   check=True, capture_output=True)
    src = tmp_path / "enums.c"
    src.write_text('#include <stdio.h>\n#include "pdsp_hip_fft2d.h"\nint main(void) {\n'
                   '  printf("%d %d %d %d %d %d\\n", PDSP_NORM_BACKWARD, PDSP_NORM_ORTHO, PDSP_NORM_FORWARD,\n'
                   '         PDSP_FFT2D_RESIDENT, PDSP_FFT2D_TWO_PASS, PDSP_FFT2D_INFO);\n  return 0;\n}\n')
    exe = str(tmp_path / "enums")
    subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", inc, "-o", exe, str(src)], check=True,
                   capture_output=True)
    assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split() == ["0", "1", "2", "0", "1", "4"]


def test_python_exports(pdsp):
    from pragma_dsp_amd import fft2d
    for name in ("Fft2d", "fft2", "ifft2"):
        assert name in pdsp.__all__ and getattr(pdsp, name) is getattr(fft2d, name)
    assert fft2d.NORMS == {None: 0, "backward": 0, "ortho": 1, "forward": 2}


def last_error(pdsp):
    return pdsp.lib.pdsp_last_error().decode()


def test_refusals_come_ahead_of_the_device_check(pdsp):
    lib = pdsp.lib
    # the handle, on both stream entry points
    for fn in (lib.pdsp_fft2d_c2c_f32, lib.pdsp_fft2d_c2c_f64):
        assert fn(None, 1, None, None, None, None, 0, 0, None) == ERR_BAD_ARG
        assert last_error(pdsp) == "fft2d is null"
    assert lib.pdsp_fft2d_destroy(None) == 0 and lib.pdsp_fft2d_height(None) == 0 and lib.pdsp_fft2d_width(None) == 0
    assert lib.pdsp_fft2d_create(64, 64, -1, None) == ERR_BAD_ARG and last_error(pdsp) == "out is null"
    h = C.c_void_p()
    assert lib.pdsp_fft2d_create(64, 48, -1, C.byref(h)) == ERR_UNSUPPORTED_SIZE and not h
    assert "16 <= H <= 512" in last_error(pdsp) and "got 64 x 48" in last_error(pdsp)
    # the host form has the stream entry points' checks in their order, with no handle to make first
    x = np.zeros((2, 64, 64))
    p = x.ctypes.data_as(C.POINTER(C.c_double))
    host = lib.pdsp_fft2d_host_f64
    assert host(p, p, 0, 64, 64, 0, 0, p, p) == ERR_BAD_ARG and last_error(pdsp) == "batch must be >= 1, got 0"
    assert host(p, p, -3, 64, 64, 0, 0, p, p) == ERR_BAD_ARG and last_error(pdsp) == "batch must be >= 1, got -3"
    for norm in (-1, 3):
        assert host(p, p, 2, 64, 64, 0, norm, p, p) == ERR_BAD_ARG
        assert last_error(pdsp) == f"2-D FFT norm must be 0 (backward), 1 (ortho) or 2 (forward), got {norm}"
    for args in ((None, p, p, p), (p, p, None, p), (p, p, p, None)):
        assert host(args[0], args[1], 2, 64, 64, 0, 0, args[2], args[3]) == ERR_BAD_ARG and last_error(pdsp) == "null buffer"
    assert host(p, None, 2, 64, 64, 1, 0, p, p) == ERR_BAD_ARG
    assert last_error(pdsp) == "the inverse needs both planes (im_in is null)"
    assert host(p, p, 2, 64, 32768, 0, 0, p, p) == ERR_UNSUPPORTED_SIZE
    # ... and the shape last, as on a handle, whose shape was settled at create
    assert host(p, p, 0, 64, 48, 0, 0, p, p) == ERR_BAD_ARG and last_error(pdsp) == "batch must be >= 1, got 0"
    assert host(p, p, 2, 64, 48, 0, 7, p, p) == ERR_BAD_ARG and "norm must be" in last_error(pdsp)
    assert host(None, p, 2, 64, 48, 0, 0, p, p) == ERR_BAD_ARG and last_error(pdsp) == "null buffer"
    assert host(p, p, 2, 64, 48, 0, 0, p, p) == ERR_UNSUPPORTED_SIZE and "got 64 x 48" in last_error(pdsp)
    # the Python layer's own
    from pragma_dsp_amd import fft2d
    with pytest.raises(pdsp.PdspError) as ei:
        fft2d.fft2(x, norm="unitary")
    assert ei.value.code == ERR_BAD_ARG and "norm must be" in str(ei.value)
    with pytest.raises(pdsp.PdspError) as ei:
        fft2d.fft2(np.zeros(64))
    assert ei.value.code == ERR_BAD_ARG


def rule(h, w, elem):
    """The decision, written out: None outside the domain, else (path, images per workgroup, tile, launches)."""
    def pow2(v):
        return v >= 1 and v & (v - 1) == 0
    wmax = 16384 if elem == 4 else 8192
    if not (pow2(h) and pow2(w) and 16 <= h <= 512 and 16 <= w <= wmax):
        return None
    if h * w <= 4096:
        return (0, 4096 // (h * w), 0, 1)
    wide = 256 if h <= 32 else 64 if h == 64 else 32 if h == 128 else (32 if elem == 4 else 16)
    return (1, 0, min(wide, w), 2)


def ask(pdsp, h, w, elem):
    info = (C.c_int * 4)(-7, -7, -7, -7)
    return pdsp.lib.pdsp_fft2d_query(h, w, elem, info), tuple(info)


def test_query_over_the_whole_domain(pdsp):
    resident = set()
    for elem in (4, 8):
        for lh in range(4, 10):
            for lw in range(4, 15 if elem == 4 else 14):
                h, w = 1 << lh, 1 << lw
                rc, info = ask(pdsp, h, w, elem)
                assert rc == 0 and info == rule(h, w, elem), (h, w, elem, info)
                if info[0] == 0:
                    resident.add((h, w))
                    assert info[1] == 4096 // (h * w) and info[3] == 1
                else:
                    assert 16 <= info[2] <= w and w % info[2] == 0 and info[3] == 2
    assert len(resident) == 15 and all(h * w <= 4096 for h, w in resident)


@pytest.mark.parametrize("h,w,elem", [(8, 64, 4), (1024, 64, 4), (64, 8, 4), (64, 32768, 4), (64, 16384, 8), (16, 16384, 8),
                                      (48, 64, 4), (64, 48, 8), (0, 64, 4), (64, 0, 4), (-64, 64, 4), (64, -64, 8),
                                      (8, 8, 8), (1024, 32768, 4)])
def test_query_refuses_the_edges_just_outside(pdsp, h, w, elem):
    assert rule(h, w, elem) is None
    rc, info = ask(pdsp, h, w, elem)
    assert rc == ERR_UNSUPPORTED_SIZE and info == (-7, -7, -7, -7), "info must stay unwritten"
    msg = last_error(pdsp)
    assert "16 <= H <= 512" in msg and "16384 in f32" in msg and "8192 in f64" in msg and f"got {h} x {w}" in msg
    assert pdsp.lib.pdsp_fft2d_query(64, 64, 2, (C.c_int * 4)()) == ERR_BAD_ARG
    assert pdsp.lib.pdsp_fft2d_query(64, 64, 4, None) == ERR_BAD_ARG and last_error(pdsp) == "null buffer"


def test_stream_entry_points_of_the_header():
    import graph_capture_cases as G
    assert G.stream_entry_points(HEADER) == ["pdsp_fft2d_c2c_f32", "pdsp_fft2d_c2c_f64"]

"""pdsp_dev_transform_path_* / pdsp_dev_spectrum_path_* themselves: queries only, no transform runs, so the cost is plan
creation.  Every pointer is a real NaN-filled device buffer (the queries only look at addresses) and every buffer is
checked to be unchanged.  Each case names the decision by its info fields (include/pdsp_hip_dev.h) and, through
path_names(), must also agree with the independent mirrors of the two path files."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_f32_paths as f32
import test_gpu_f64_paths as f64

pytestmark = pytest.mark.gpu

STOCKHAM, SPLIT4, REAL_PACKED, PAIRED, TILES, FOURSTEP, DIF16K, PACKED = 3, 5, 6, 7, 8, 9, 14, 15


@pytest.fixture(scope="module", autouse=True)
def _release_plans():
    yield
    for mod in (f32, f64):
        for p in mod._PLANS.values():
            p.close()
        mod._PLANS.clear()


def _info(fn, *args):
    info = (C.c_int * f32.PATH_INFO)(*([-1] * f32.PATH_INFO))
    assert fn(*args, info) == 0, f32._lib().pdsp_last_error()
    return list(info)


def _with(setter, value, ask):
    lib = f32._lib()
    prev = getattr(lib, setter)(value)
    try:
        return ask()
    finally:
        getattr(lib, setter)(prev)


def _untouched(*bufs):
    import torch
    for b in bufs:
        assert bool(torch.isnan(b.flat).all()), "a query wrote to a buffer"


def test_transform_queries_f32():
    lib = f32._lib()
    q = lib.pdsp_dev_transform_path_f32
    n, batch = 16384, 2
    p = f32.plan(n)._h
    re, im, ore, oim = (f32.Buf(batch, n, 0) for _ in range(4))
    re1, ore1, oim1 = f32.Buf(batch, n, 1), f32.Buf(batch, n, 1), f32.Buf(batch, n, 1)
    aligned = lambda: _info(q, p, batch, re.ptr, im.ptr, ore.ptr, oim.ptr, 0)  # noqa: E731
    assert aligned()[:2] == [SPLIT4, SPLIT4]
    assert _info(q, p, batch, re1.ptr, im.ptr, ore.ptr, oim.ptr, 0)[0] == STOCKHAM
    assert _with("pdsp_set_split16k", 0, aligned)[0] == STOCKHAM
    assert aligned()[0] == SPLIT4  # the switch is back
    assert _info(q, p, batch, re.ptr, im.ptr, ore1.ptr, oim1.ptr, 0)[0] == SPLIT4
    assert _info(q, p, batch, re.ptr, im.ptr, ore.ptr, oim.ptr, 1)[0] == SPLIT4  # inverse: the same planes exchanged
    assert f32.path_names(aligned(), n) == f32.expected_path("complex", n, batch, (0, 0, 0, 0))
    _untouched(re, im, ore, oim, re1, ore1, oim1)

    n = 1 << 15
    p = f32.plan(n)._h
    re, im, ore, oim = (f32.Buf(batch, n, 0) for _ in range(4))
    re1 = f32.Buf(batch, n, 1)
    disjoint = lambda: _info(q, p, batch, re.ptr, im.ptr, ore.ptr, oim.ptr, 0)  # noqa: E731
    assert disjoint()[0] == PAIRED
    inplace = _info(q, p, batch, re.ptr, im.ptr, re.ptr, im.ptr, 0)
    assert inplace[0] == TILES and inplace[4] == 2 and inplace[9] == 1 and inplace[10] == 0  # np, pairs, out_first
    assert f32.path_names(inplace, n) == f32.expected_path("complex", n, batch, (0, 0, 0, 0), aliasing=True)
    assert _info(q, p, batch, re1.ptr, im.ptr, ore.ptr, oim.ptr, 0)[0] == FOURSTEP
    tp5 = _with("pdsp_set_twopass", 5, disjoint)
    assert tp5[0] == TILES and tp5[4] == 2
    assert f32.path_names(tp5, n) == f32.expected_path("complex", n, batch, (0, 0, 0, 0), switches={"twopass": 5})
    assert _with("pdsp_set_twopass", 0, disjoint)[0] == FOURSTEP
    assert disjoint()[0] == PAIRED
    _untouched(re, im, ore, oim, re1)


def test_spectrum_queries_f32():
    lib = f32._lib()
    q = lib.pdsp_dev_spectrum_path_f32
    n, batch = 16384, 2
    pl = f32.plan(n)
    p, hann = pl._h, pl.window("hann").data_ptr()
    frames = f32.Buf(batch, n + 1, 0)  # one float more per frame, for the odd stride
    table = f32.Buf(1, n, 0)           # a caller's table (its values are never read)
    amp, ph = f32.Buf(batch, n), f32.Buf(batch, n)
    mirror = lambda **kw: f32.expected_path("spectrum", n, batch, (0, 0), **dict(  # noqa: E731
        dict(frame_len=n, stride=n, window=("plan", "hann"), sides="one", outputs={"amp"}), **kw))
    base = lambda: _info(q, p, batch, frames.ptr, n, n, hann, 0, amp.ptr, None, None, None, 1.0)  # noqa: E731
    b = base()
    assert b[0] == DIF16K and b[11] == 1 and b[12] == 2  # fast, the fused two-term window
    assert f32.path_names(b, n, True) == mirror() == {"spectrum_dif16k_kernel-w2"}
    moved = {
        "phase": (_info(q, p, batch, frames.ptr, n, n, hann, 0, amp.ptr, ph.ptr, None, None, 1.0),
                  mirror(outputs={"amp", "ph"})),
        "odd stride": (_info(q, p, batch, frames.ptr, n, n + 1, hann, 0, amp.ptr, None, None, None, 1.0),
                       mirror(stride=n + 1)),
        "frame_len N - 2": (_info(q, p, batch, frames.ptr, n - 2, n, hann, 0, amp.ptr, None, None, None, 1.0),
                            mirror(frame_len=n - 2)),
        "two-sided": (_info(q, p, batch, frames.ptr, n, n, hann, 1, amp.ptr, None, None, None, 1.0),
                      mirror(sides="two")),
    }
    for what, (info, want) in moved.items():
        assert info[0] == PACKED and info[11] == 0 and info[12] == 1, (what, info)  # general, the window as a table
        assert f32.path_names(info, n, True) == want, (what, info)
        assert "spectrum_packed-16384-general" in want, what
    tab = _info(q, p, batch, frames.ptr, n, n, table.ptr, 0, amp.ptr, None, None, None, 1.0)
    assert tab[0] == DIF16K and tab[12] == 1
    assert f32.path_names(tab, n, True) == mirror(window=("table", "hann")) == {"spectrum_dif16k_kernel-w1"}
    off = _with("pdsp_set_fused_window", 0, base)
    assert off[0] == DIF16K and off[12] == 1
    assert f32.path_names(off, n, True) == mirror(switches={"fused_window": 0})
    assert base() == b  # the switch is back
    _untouched(frames, table, amp, ph)


def test_transform_queries_f64_real_rows():
    lib = f32._lib()
    q = lib.pdsp_dev_transform_path_f64
    n = 16384
    p = f64.plan(n)._h
    re, ore, oim = (f64.dbuf(8, n, 0) for _ in range(3))
    b7 = _info(q, p, 7, re.ptr, None, ore.ptr, oim.ptr, 0)
    b8 = _info(q, p, 8, re.ptr, None, ore.ptr, oim.ptr, 0)
    assert b7[0] == FOURSTEP and b8[0] == REAL_PACKED
    assert f64.path_names_f64(b7, n) == f64.expected_path_f64("real", n, 7, (0, None, 0, 0))
    assert f64.path_names_f64(b8, n) == f64.expected_path_f64("real", n, 8, (0, None, 0, 0))
    assert _with("pdsp_set_real_packed", 0, lambda: _info(q, p, 8, re.ptr, None, ore.ptr, oim.ptr, 0))[0] == FOURSTEP
    _untouched(re, ore, oim)
    n = 8192
    p = f64.plan(n)._h
    re, re1, ore, oim = f64.dbuf(3, n, 0), f64.dbuf(3, n, 1), f64.dbuf(3, n, 0), f64.dbuf(3, n, 0)
    assert _info(q, p, 3, re.ptr, None, ore.ptr, oim.ptr, 0)[0] == REAL_PACKED
    off1 = _info(q, p, 3, re1.ptr, None, ore.ptr, oim.ptr, 0)
    assert off1[0] == STOCKHAM
    assert f64.path_names_f64(off1, n) == f64.expected_path_f64("real", n, 3, (1, None, 0, 0))
    _untouched(re, re1, ore, oim)

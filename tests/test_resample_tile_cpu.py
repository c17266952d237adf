"""The rate-change kernels' tile rule (upfirdn_tile, pdsp_kernels_resample.hip) without a device, through
the development query pdsp_dev_upfirdn_tile: over a grid of the whole supported domain and seeded random points, the
tile the rule reports is held to what the KERNEL needs, restated here from pdsp_upfirdn_kernel.h and not from the rule:
the highest and lowest sample index any item reads lie inside the staged span and its 8 front zeros, the LDS size is
the layout's, and every in-tile 32-bit product stays below 2^31.  Then the pins DESIGN.md 4.9 names, and the switch
pdsp_set_upfirdn_tile: each forced instantiation is the one reported or the call fails, the cap on B holds, and the
same index ranges hold for every forced and capped tile (the GPU tests run those: tests/test_gpu_resample_paths.py)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from pragma_dsp_amd import _capi
from pragma_dsp_amd._capi import lib

VALUES = [1, 2, 3, 4, 7, 8, 16, 63, 64, 147, 160, 255, 256, 257, 400, 1023, 1024, 2048, 2731, 4095, 4096, 4097, 8191,
          8192]
Y_LENS = [1, 5, 300, 5000, 100000, 10 ** 9]
FRONT, LDS_MAX, SPAN_MAX = 8, 163840, 40960
R_OF = {1: 4, 2: 8, 3: 1, 4: 1}              # pdsp_set_upfirdn_tile's instantiations: r,
WIN_GT_OF = {1: (0, 0), 2: (1, 0), 3: (0, 0), 4: (0, 1)}  # win and gt


@pytest.fixture
def tile_mode():
    """Sets the process-wide switch; the production rule is back whatever the test did."""
    try:
        yield lib.pdsp_set_upfirdn_tile
    finally:
        lib.pdsp_set_upfirdn_tile(0)


def query(up, down, ntaps, y_len, elem):
    """(status, info) of one point."""
    info = (C.c_longlong * 9)()
    rc = lib.pdsp_dev_upfirdn_tile(up, down, ntaps, y_len, elem, info)
    return rc, tuple(info)


def query_all(points):
    """points: int64 [n, 5] of up, down, ntaps, y_len, elem -> (status [n], info [n, 9])."""
    info = (C.c_longlong * 9)()
    view = np.frombuffer(info, dtype=np.int64)
    out = np.zeros((len(points), 9), dtype=np.int64)
    rcs = np.zeros(len(points), dtype=np.int64)
    fn = lib.pdsp_dev_upfirdn_tile
    for i, (up, down, ntaps, y_len, elem) in enumerate(points.tolist()):
        rcs[i] = fn(up, down, ntaps, y_len, elem, info)
        out[i] = view
    return rcs, out


def grid_points():
    return np.array(list(itertools.product(VALUES, VALUES, VALUES, Y_LENS, (4, 8))), dtype=np.int64)


def random_points(n, seed):
    rng = np.random.default_rng(seed)
    dims = np.where(rng.random((n, 3)) < 0.5, rng.integers(1, 8193, (n, 3)),       # uniform, and
                    np.exp(rng.uniform(0, np.log(8192.999), (n, 3))).astype(np.int64))  # as many small as large
    y_len = np.exp(rng.uniform(0, np.log(2e9), (n, 1))).astype(np.int64)
    elem = rng.choice([4, 8], (n, 1))
    return np.concatenate([np.clip(dims, 1, 8192), np.maximum(y_len, 1), elem], axis=1).astype(np.int64)


def hold_to_the_kernel(points, info):
    """Every invariant of a reported tile, all points at once.  Python ints would be exact; int64 is enough: the
    largest product below is 8192 * 8192 * 8193 < 2^40."""
    up, down, ntaps, y_len, elem = points.T
    r, win, gt, tn, tp, bper, span, lds, items = info.T
    where = lambda bad: points[bad][:3].tolist()  # noqa: E731
    assert np.all(tn == -(-ntaps // up)), where(tn != -(-ntaps // up))
    assert np.all((tp == tn) | (tp == tn + 1))
    assert np.all(np.isin(r, (1, 4, 8)))
    assert np.all((bper >= r) & (bper % r == 0))
    assert np.all((win == 0) | ((r == 8) & (down == 1)))
    assert np.all((gt == 0) | (r == 1))
    assert np.all((win == 0) | (gt == 0))
    assert np.all(items == up * bper // r)
    taps_lds = np.where(gt == 1, 0, up * tp)
    assert np.all(lds == (taps_lds + FRONT + span) * elem)
    assert np.all(lds <= LDS_MAX), where(lds > LDS_MAX)
    assert np.all(span <= SPAN_MAX), where(span > SPAN_MAX)
    # pdsp_upfirdn_kernel.h: an item of phase step a < up starts at qa = p_lo + a down, p_lo <= up - 1, ka = qa div up
    ka_max = (up - 1 + (up - 1) * down) // up
    # WIN = false: xl[ka + b down + tn - 1 - j], b = bg + i groups < bper, j < tn
    hi_plain = ka_max + (bper - 1) * down + tn - 1
    lo_plain = np.zeros_like(tn)                         # ka = 0, b = 0, j = tn - 1
    # WIN = true: preloads xl[ka + bg R + tn - 1 + i], i < R, bg < bper / R; then one sample per step j < roundup(tn, R)
    # at xl[ka + bg R + tn - 1 - (j + 1)]
    hi_win = ka_max + (bper // r - 1) * r + tn - 1 + (r - 1)
    lo_win = tn - 1 - (-(-tn // r)) * r
    hi = np.where(win == 1, hi_win, hi_plain)
    lo = np.where(win == 1, lo_win, lo_plain)
    assert np.all(hi < span), where(hi >= span)
    assert np.all(lo >= -FRONT), where(lo < -FRONT)
    # the taps: row p < up, entries j < tn, at stride tp in LDS or (GT) at stride tn in the table of up * tn values
    assert np.all(np.where(gt == 1, (up - 1) * tn + tn - 1 < up * tn, (up - 1) * tp + tn - 1 < taps_lds))
    for prod in (up * tp, up * tn, (up - 1) * down + up - 1, bper * down, up * bper):
        assert np.all(prod < 2 ** 31)
    assert np.all(up * bper >= 1)


@pytest.fixture(scope="module")
def ruled():
    """The rule's own tile at every grid point and 4000 random ones."""
    assert lib.pdsp_set_upfirdn_tile(0) == 0
    points = np.concatenate([grid_points(), random_points(4000, 20240901)])
    rcs, info = query_all(points)
    return points, rcs, info


def test_the_rule_gives_every_point_of_the_domain_a_tile_the_kernel_can_run(ruled):
    points, rcs, info = ruled
    assert len(points) == 24 ** 3 * 6 * 2 + 4000
    assert np.all(rcs == 0), points[rcs != 0][:3].tolist()
    hold_to_the_kernel(points, info)


def test_the_rule_never_reads_f32_taps_from_global_memory(ruled):
    """The finding: an f32 tap table and one span always fit 160 KiB, so upfirdn_kernel<float, 1, false, true> runs
    only where pdsp_set_upfirdn_tile forces it.  The f64 one is chosen, for tables near 64 KiB at down near 8192."""
    points, _, info = ruled
    f32 = points[:, 4] == 4
    assert not np.any(info[f32, 2])
    assert np.any(info[~f32, 2])
    # it is chosen exactly where the layout of an R = 1 tile of one output per phase, taps in LDS, exceeds 160 KiB
    up, down, ntaps, _, elem = points.T
    tn = -(-ntaps // up)
    least = up * tn + FRONT + tn + (up - 1 + (up - 1) * down) // up
    assert np.array_equal(info[:, 2] == 1, least * elem > LDS_MAX)


def test_every_instantiation_is_chosen_somewhere(ruled):
    _, _, info = ruled
    assert {tuple(t) for t in np.unique(info[:, :3], axis=0).tolist()} == {(4, 0, 0), (8, 1, 0), (1, 0, 0), (1, 0, 1)}


def test_the_tiles_design_md_names(tile_mode):
    """DESIGN.md 4.9's table of pins."""
    for elem in (4, 8):
        rc, t = query(2, 1, 41, 1 << 17, elem)
        assert rc == 0 and t[:3] == (8, 1, 0)                      # 2/1 with its 41 default taps: WIN
        rc, t = query(1, 8, 161, 8192, elem)
        assert rc == 0 and t[:3] == (4, 0, 0)                      # 1/8, 161 taps: R = 4
        rc, t = query(1, 400, 8001, 50, elem)
        assert rc == 0 and t[:3] == (1, 0, 0)                      # 1/400, 8001 taps, 50 outputs: R = 1
        rc, t = query(1, 63, 17, 301, elem)
        assert rc == 0 and t[:3] == (4, 0, 0) and t[7] > 65536     # R = 4 above the default dynamic-LDS limit
    for y_len in (1, 3, 8193, 19999):
        rc, t = query(8191, 8192, 8192, y_len, 8)
        assert rc == 0 and t[:3] == (1, 0, 1) and t[3] == 2         # f64 8191/8192, 8192 taps: GT
        rc, t = query(8191, 8192, 8192, y_len, 4)
        assert rc == 0 and t[:3] == (1, 0, 0)
    rc, t = query(4096, 8192, 8192, 5, 8)
    assert rc == 0 and t[:3] == (1, 0, 0) and t[3:5] == (2, 2)      # f64 4096/8192: R = 1, the unpadded tap stride
    rc, t = query(4096, 8192, 8192, 5, 4)
    assert rc == 0 and t[:3] == (1, 0, 0) and t[3:5] == (2, 3)      # f32: R = 1, padded


def test_the_setter_returns_the_previous_value_and_leaves_junk_out(tile_mode):
    assert tile_mode(3) == 0
    assert tile_mode((5 << 4) | 1) == 3
    for junk in (-1, 5, 15, (2 << 4) | 7, -(1 << 31)):
        assert tile_mode(junk) == (5 << 4) | 1       # unchanged, and said so
    assert tile_mode(7 << 4) == (5 << 4) | 1         # a cap alone: the rule among capped tiles
    assert tile_mode(0) == 7 << 4
    assert tile_mode(0) == 0


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_a_forced_instantiation_is_the_one_reported_or_the_call_fails(mode, tile_mode):
    rng = np.random.default_rng(mode)
    sub = grid_points()
    sub = sub[rng.choice(len(sub), 6000, replace=False)]
    no_room = np.array([(8191, 8192, 8192, 3, 8), (4095, 8192, 8192, 300, 8), (8191, 4096, 8192, 5000, 8)])
    points = np.concatenate([sub, random_points(1500, mode), no_room])  # the last: f64 tap tables that leave no room
    if mode == 2:
        points[::2, 1] = 1  # WIN is legal at down == 1 only: half of the points
    tile_mode(mode)
    rcs, info = query_all(points)
    ok = rcs == 0
    assert np.all((rcs == 0) | (rcs == _capi.ERR_UNSUPPORTED_SIZE))
    assert np.all(info[ok, 0] == R_OF[mode])
    assert np.all(info[ok, 1] == WIN_GT_OF[mode][0]) and np.all(info[ok, 2] == WIN_GT_OF[mode][1])
    hold_to_the_kernel(points[ok], info[ok])
    if mode == 2:
        assert np.array_equal(ok, points[:, 1] == 1)  # every down == 1 fits: the tap table is at most 64 KiB + pad
    if mode == 4:
        assert np.all(ok)                             # a span alone always fits
    if mode in (1, 3):
        assert ok.sum() > len(points) // 2 and not np.all(ok)
        # what fails has no tile of one R-group within 160 KiB, computed here from the layout
        up, down, ntaps, _, elem = points[~ok].T
        tn = -(-ntaps // up)
        r = R_OF[mode]
        least = up * tn + FRONT + tn + (up - 1 + (up * r - 1) * down) // up
        assert np.all(least * elem > LDS_MAX)


def test_a_forced_instantiation_fails_by_name_and_is_never_replaced(tile_mode):
    name = {1: "R = 4", 2: "R = 8, WIN", 3: "R = 1", 4: "R = 1, GT"}
    tile_mode(2)
    rc, _ = query(3, 2, 17, 300, 4)
    msg = lib.pdsp_last_error().decode()
    assert rc == _capi.ERR_UNSUPPORTED_SIZE and name[2] in msg and "down == 1" in msg
    for mode in (1, 3):  # f64 8191/8192 with 8192 taps: the tap table leaves no room
        tile_mode(mode)
        rc, _ = query(8191, 8192, 8192, 3, 8)
        msg = lib.pdsp_last_error().decode()
        assert rc == _capi.ERR_UNSUPPORTED_SIZE and name[mode] + ")" in msg and "160 KiB" in msg
    tile_mode(4)
    rc, t = query(8191, 8192, 8192, 3, 8)
    assert rc == 0 and t[:3] == (1, 0, 1)
    rc, t = query(3, 2, 17, 300, 4)
    assert rc == 0 and t[:3] == (1, 0, 1)  # f32 GT: only this way


@pytest.mark.parametrize("cap", [1, 3, 8, 9, 100])
@pytest.mark.parametrize("inst", [0, 1, 2, 3, 4])
def test_the_cap_on_b_holds(inst, cap, tile_mode):
    points = random_points(1500, 100 * cap + inst)
    if inst == 2:
        points[:, 1] = 1
    tile_mode(0 if inst == 0 else inst)
    rcs0, free = query_all(points)
    tile_mode((cap << 4) | inst)
    rcs, info = query_all(points)
    assert np.array_equal(rcs, rcs0)  # a smaller tile fits wherever a larger one did, and nothing else does
    ok = rcs == 0
    r, bper = info[ok, 0], info[ok, 5]
    assert np.all(bper <= -(-cap // r) * r)
    hold_to_the_kernel(points[ok], info[ok])
    if inst:
        assert np.all(info[ok, :5] == free[ok, :5])  # a cap and nothing else


def test_the_query_validates_its_arguments(tile_mode):
    info = (C.c_longlong * 9)(*([-7] * 9))
    bad, unsup = _capi.ERR_BAD_ARG, _capi.ERR_UNSUPPORTED_SIZE
    for args, code in (((0, 1, 17, 5, 4), bad), ((1, 0, 17, 5, 4), bad), ((1, 1, 0, 5, 4), bad), ((1, 1, 17, 0, 4), bad),
                       ((1, 1, 17, -1, 8), bad), ((1, 1, 17, 5, 2), bad), ((1, 1, 17, 5, 16), bad),
                       ((8193, 1, 17, 5, 4), unsup), ((1, 8193, 17, 5, 4), unsup), ((1, 1, 8193, 5, 4), unsup)):
        assert lib.pdsp_dev_upfirdn_tile(*args, info) == code and lib.pdsp_last_error()
        assert list(info) == [-7] * 9
    assert lib.pdsp_dev_upfirdn_tile(1, 1, 17, 5, 4, None) == bad

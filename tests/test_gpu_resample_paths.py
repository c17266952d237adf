"""Polyphase rate change on the GPU, instantiation by instantiation.  The tile rule picks one of four
upfirdn_kernel instantiations per precision; pdsp_set_upfirdn_tile (pdsp_hip_dev.h) forces one and caps the tile, and
pdsp_dev_upfirdn_tile reports what a call runs.  Every test here asks the query, under the very switch value of the
call, which instantiation and how many tiles ran, and holds the outputs to the bound of tests/test_gpu_resample.py,

    |y[m] - ref[m]| <= (T + 2) * eps * A[m],   T = ceil(ntaps / up),  A[m] = sum |h| |x| over the output's terms,

nothing excluded, exactly 0 where A[m] == 0 -- against the gather-form f64 reference of tests/test_resample_cpu.py
(pinned there to the zero-stuffing one), which reaches up = 8191.  Forced and capped runs must also equal the rule's
own output bit for bit: every output is the same fmas in the same order in every instantiation and tile.
Each case prints its worst share of the bound (pytest -s)."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest
import torch

import pragma_dsp_amd as pd
from pragma_dsp_amd import _capi
from pragma_dsp_amd._capi import lib
from test_gpu_resample import DTYPES, EPS, NP, dev, signal
from test_resample_cpu import resample_ref_direct, user_taps

pytestmark = pytest.mark.gpu

Tile = namedtuple("Tile", "r win gt tn tp bper span lds_bytes items tiles")
R4, WIN, R1, GT = (4, 0, 0), (8, 1, 0), (1, 0, 0), (1, 0, 1)  # (r, win, gt) of pdsp_set_upfirdn_tile's 1 ... 4
INST = {1: R4, 2: WIN, 3: R1, 4: GT}
ELEM = {torch.float32: 4, torch.float64: 8}


@pytest.fixture
def tile_mode():
    """Sets the process-wide switch; the production rule is back whatever the test did."""
    try:
        yield lib.pdsp_set_upfirdn_tile
    finally:
        lib.pdsp_set_upfirdn_tile(0)


def tile_of(up, down, ntaps, y_len, dt):
    """What a launch with these arguments runs under the switch as it is now."""
    info = (C.c_longlong * 9)()
    _capi.check(lib.pdsp_dev_upfirdn_tile(up, down, ntaps, y_len, ELEM[dt], info))
    t = tuple(info)
    return Tile(*t, tiles=-(-y_len // (up * t[5])))


def hold(y, x, up, down, taps, t0, dt, what):
    """y: [rows, y_len] device outputs of x ([rows, len], f64 values exact in dt) -> held to the bound."""
    got = y.cpu().numpy().astype(np.float64)
    h = np.asarray(taps, dtype=np.float64).astype(NP[dt]).astype(np.float64)  # as the handle rounds them
    ref = resample_ref_direct(x, up, down, h, t0, got.shape[1])
    a = resample_ref_direct(x, up, down, h, t0, got.shape[1], abs=True)
    bound = (-(-h.size // up) + 2) * EPS[dt] * a
    err = np.abs(got - ref)
    worst = float((err[a > 0] / bound[a > 0]).max()) if (a > 0).any() else 0.0
    print(f"{what} {dt} len {x.shape[1]}: worst |err| / bound = {worst:.3f}")
    assert got.shape == ref.shape
    assert np.all(got[a == 0] == 0.0)
    assert np.all(err <= bound), (what, worst)
    return a


FORCED = [(3, 2, 17, 300), (3, 2, 16, 300), (1, 3, 17, 300), (7, 5, 3, 100), (2, 1, 41, 300), (5, 1, 8, 64)]


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("up,down,ntaps,n", FORCED)
def test_every_forced_instantiation_in_one_tile_and_in_many(up, down, ntaps, n, dt, tile_mode):
    """(3, 2, 16): even T at up > 1, the padded tap stride; (7, 5, 3): phases without a tap; cap 1 = one R-group per
    phase and tile, tens of tiles with a 64-bit origin and a non-zero phase each.  The first run there is of
    upfirdn_kernel<float, 1, false, true>, which the rule never picks."""
    r = pd.Upfirdn(user_taps(ntaps), up, down, device="cuda:0", dtype=dt)
    x = signal((3, n), dt, 1000 * up + ntaps)
    xd = dev(x, dt)
    y_len = r.output_len(n)
    ruled = tile_of(up, down, ntaps, y_len, dt)
    want = r.apply(xd)
    hold(want, x, up, down, r.taps, 0, dt, f"rule {ruled[:3]} {up}/{down} taps {ntaps}")
    ran = set()
    for inst in (1, 2, 3, 4) if down == 1 else (1, 3, 4):
        for cap in (1, 0):
            tile_mode((cap << 4) | inst)
            t = tile_of(up, down, ntaps, y_len, dt)
            assert t[:3] == INST[inst]
            assert t.tn == -(-ntaps // up) and t.tp == (t.tn + 1 if up > 1 and t.tn % 2 == 0 else t.tn)
            if cap:
                assert t.bper == t.r and t.tiles == -(-y_len // (up * t.r)) >= 2
            y = r.apply(xd)
            torch.cuda.synchronize()
            assert torch.equal(y, want), (inst, cap)
            hold(y, x, up, down, r.taps, 0, dt, f"forced {t[:3]} x {t.tiles} tiles, {up}/{down} taps {ntaps}")
            ran.add(t[:3])
    assert ran == ({R4, WIN, R1, GT} if down == 1 else {R4, R1, GT})


def test_a_forced_instantiation_that_cannot_run_is_refused_not_replaced(tile_mode):
    r = pd.Upfirdn(user_taps(17), 3, 2, device="cuda:0")
    x = torch.ones(2, 100, device="cuda")
    out = torch.full((2, r.output_len(100)), float("nan"), device="cuda")
    tile_mode(2)  # WIN needs down == 1
    with pytest.raises(pd.PdspError) as e:
        r.apply(x, out=out)
    assert e.value.code == _capi.ERR_UNSUPPORTED_SIZE and "R = 8, WIN" in str(e.value)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()  # before any launch
    tile_mode(0)
    assert torch.equal(r.apply(x, out=out), r.apply(x))


@pytest.mark.parametrize("n,tiles", [(20000, 3), (8193, 2), (1, 1)])
def test_f64_taps_from_global_memory_as_the_rule_picks_it(n, tiles):
    """8192 taps at 8191/8192: 64 KiB of taps leave no room for a span of 64 KiB.  Rows of 20000: three tiles of 8191
    outputs (origins 0, 8191 * 8192 and twice that; phases 0, 1, 2); of 8193: a last tile of one output."""
    dt = torch.float64
    h = user_taps(8192)
    r = pd.Upfirdn(h, 8191, 8192, device="cuda:0", dtype=dt)
    y_len = r.output_len(n)
    t = tile_of(8191, 8192, 8192, y_len, dt)
    assert t[:3] == GT and t.bper == 1 and t.tiles == tiles and y_len - (tiles - 1) * 8191 >= 1
    if n >= 8193:
        assert t.lds_bytes > 65536
    if n == 8193:
        assert y_len == 8191 + 1
    x = signal((3, n), dt, n)
    hold(r.apply(dev(x, dt)), x, 8191, 8192, h, 0, dt, f"rule GT x {tiles} tiles")


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_r4_above_the_default_dynamic_lds_limit(dt):
    h = user_taps(17)
    r = pd.Upfirdn(h, 1, 63, device="cuda:0", dtype=dt)
    n = 18900
    t = tile_of(1, 63, 17, r.output_len(n), dt)
    assert t[:3] == R4 and t.lds_bytes > 65536 and r.output_len(n) == 301
    x = signal((3, n), dt, 63)
    hold(r.apply(dev(x, dt)), x, 1, 63, h, 0, dt, f"rule R = 4, {t.lds_bytes} bytes of LDS")


def test_the_unpadded_tap_stride():
    """f64 4096/8192 with 8192 taps: T = 2 would be padded to a stride of 3, which does not fit: R = 1, tp == tn."""
    dt = torch.float64
    h = user_taps(8192)
    r = pd.Upfirdn(h, 4096, 8192, device="cuda:0", dtype=dt)
    t = tile_of(4096, 8192, 8192, r.output_len(9), dt)
    assert t[:3] == R1 and t.tp == t.tn == 2
    assert tile_of(4096, 8192, 8192, r.output_len(9), torch.float32).tp == 3
    x = signal((3, 9), dt, 4096)
    hold(r.apply(dev(x, dt)), x, 4096, 8192, h, 0, dt, "rule R = 1, tp == tn")


def upfirdn_abi(handle, x, y, y_len, dt):
    """pdsp_upfirdn_* on the rows of x into the first y_len columns of y's rows."""
    fn = lib.pdsp_upfirdn_f32 if dt == torch.float32 else lib.pdsp_upfirdn_f64
    _capi.check(fn(handle, x.shape[0], C.c_void_p(x.data_ptr()), x.shape[1], x.stride(0), C.c_void_p(y.data_ptr()),
                   y_len, y.stride(0), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("up,down", [(3, 2), (1, 4)])
def test_any_t0_and_any_y_len_through_the_c_abi(up, down, dt, tile_mode):
    ntaps, n = 17, 300
    h = user_taps(ntaps)
    x = signal((3, n), dt, up + down)
    xd = dev(x, dt)
    for t0 in sorted({0, 1, up - 1, up, ntaps + up - 1}):
        handle = C.c_void_p()
        _capi.check(lib.pdsp_resampler_create(0, up, down, _capi.dptr(h), ntaps, t0, C.byref(handle)))
        try:
            natural = -(-((n - 1) * up + ntaps - t0) // down)  # outputs with a term: t0 + m down < (n - 1) up + ntaps
            assert natural > 47
            first = None
            for mode in (0, 1, 3):
                tile_mode(mode)
                t = tile_of(up, down, ntaps, natural, dt)
                assert mode == 0 or t[:3] == INST[mode]
                buf = torch.full((4, natural + 50), float("nan"), dtype=dt, device="cuda")
                upfirdn_abi(handle, xd, buf, natural, dt)
                a = hold(buf[:3, :natural], x, up, down, h, t0, dt, f"t0 {t0} mode {mode} {up}/{down}")
                assert np.all(a[:, natural - 1] > 0) and torch.isnan(buf[:3, natural:]).all() and torch.isnan(buf[3]).all()
                first = buf if first is None else first
                assert torch.equal(buf[:3, :natural], first[:3, :natural])
                short = torch.full_like(buf, float("nan"))
                upfirdn_abi(handle, xd, short, natural - 7, dt)
                assert torch.equal(short[:3, :natural - 7], buf[:3, :natural - 7])
                assert torch.isnan(short[:3, natural - 7:]).all() and torch.isnan(short[3]).all()
                longer = torch.full_like(buf, float("nan"))
                upfirdn_abi(handle, xd, longer, natural + 40, dt)
                hold(longer[:3, :natural + 40], x, up, down, h, t0, dt, f"t0 {t0} mode {mode} {up}/{down} + 40")
                assert torch.equal(longer[:3, :natural], buf[:3, :natural])
                assert torch.equal(longer[:3, natural:natural + 40], torch.zeros(3, 40, dtype=dt, device="cuda"))
                assert torch.isnan(longer[:3, natural + 40:]).all() and torch.isnan(longer[3]).all()
        finally:
            lib.pdsp_resampler_destroy(handle)


@pytest.mark.parametrize("mode", [3, 4])
def test_the_host_forms_run_the_forced_instantiation_too(mode, tile_mode):
    dt = torch.float64
    h = user_taps(17)
    x = signal((3, 300), dt, mode)
    poly = pd.Resampler(3, 2, device="cuda:0", dtype=dt)
    want_u = pd.Upfirdn(h, 3, 2, device="cuda:0", dtype=dt).apply(dev(x, dt)).cpu().numpy()
    want_p = poly.apply(dev(x, dt)).cpu().numpy()
    assert tile_of(3, 2, 17, want_u.shape[1], dt)[:3] == tile_of(3, 2, poly.ntaps, want_p.shape[1], dt)[:3] == R4
    tile_mode(mode)
    assert tile_of(3, 2, 17, want_u.shape[1], dt)[:3] == tile_of(3, 2, poly.ntaps, want_p.shape[1], dt)[:3] == INST[mode]
    assert np.array_equal(pd.upfirdnHost(h, x, 3, 2), want_u)
    assert np.array_equal(pd.resamplePoly(x, 3, 2), want_p)

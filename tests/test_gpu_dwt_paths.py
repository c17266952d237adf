"""Both paths of the wavelet kernels, and many small tiles, on small rows: pdsp_set_dwt_tile forces the tiled path with
T capped to 2^J and to a few multiples of it (tens of tiles, a partial last tile, halos that cross the row's end and
halos longer than the row, which wrap more than once), and the resident path where the rule would tile.
pdsp_dev_dwt_tile, asked under the same value, says what ran.  Every forced result must equal the rule's own output
bit for bit, in both directions, and is held to the bounds of test_gpu_dwt as well.  The refusals are checked as error
codes only: nothing that is refused is launched."""
import ctypes as C

import numpy as np
import pytest
import torch

import pragma_dsp_amd as pd
from pragma_dsp_amd import _capi
from test_gpu_dwt import DTYPES, case, dev, hold, host, wavelet

pytestmark = pytest.mark.gpu

EB = {torch.float32: 4, torch.float64: 8}


@pytest.fixture
def tile_switch():
    prev = pd.lib.pdsp_set_dwt_tile(0)
    yield pd.lib.pdsp_set_dwt_tile
    pd.lib.pdsp_set_dwt_tile(prev)


def tile(f, levels, n, dt, inverse):
    info = (C.c_longlong * 5)()
    assert pd.lib.pdsp_dev_dwt_tile(f, levels, n, EB[dt], int(inverse), info) == 0, pd.lib.pdsp_last_error()
    return dict(zip(("resident", "tile", "halo", "lds", "tiles"), info))


def both(w, cs, dt):
    return w.forward(dev(cs["x"], dt)), w.inverse(dev(cs["c"], dt))


# (n, J, wavelet, caps in units of 2^J): db2 and db4 with halos that cross the row's end; 32 taps at n = 96, J = 3:
# the forward halo, 210 samples, is longer than the row; caps that do not divide the row leave a partial last tile
FORCED = [
    (96, 3, "db2", (1, 2, 5)), (96, 5, "db4", (1, 2)), (96, 3, "f32", (1, 3, 5)), (208, 4, "db10", (1, 3)),
    (1024, 3, "db4", (1, 4, 13)), (1024, 6, "f6", (1, 3)), (1024, 1, "haar", (1, 7)),
]


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n,levels,key,caps", FORCED, ids=[f"{n}-{j}-{k}" for n, j, k, _ in FORCED])
def test_forced_tiles_give_the_rules_bits(tile_switch, n, levels, key, caps, dt):
    cs = case(n, levels, key, dt, 3)
    f = cs["h"].size
    w = pd.Dwt(wavelet(key), levels, "cuda:0", dt)
    assert tile(f, levels, n, dt, False)["resident"] == 1 and tile(f, levels, n, dt, True)["resident"] == 1
    fwd, inv = both(w, cs, dt)
    what = f"{key} n {n} J {levels} {dt}"
    hold(host(fwd), cs["fwd"], cs["fwd_bound"], what + " rule forward")
    hold(host(inv), cs["inv"], cs["inv_bound"], what + " rule inverse")
    for cap in (0,) + tuple(caps):
        tile_switch(2 | ((cap << levels) << 2))
        tf, ti = tile(f, levels, n, dt, False), tile(f, levels, n, dt, True)
        want = min(cap << levels, n) if cap else n  # uncapped, the rule's tile exceeds these rows
        assert (tf["resident"], tf["tile"], tf["halo"]) == (0, want, (f - 2) * ((1 << levels) - 1))
        assert (ti["resident"], ti["tile"], ti["halo"]) == (0, want, f - 2)
        assert tf["tiles"] == ti["tiles"] == -(-n // want)
        got_f, got_i = both(w, cs, dt)
        torch.cuda.synchronize()
        print(f"{what} T {want}: {tf['tiles']} tiles, halo {tf['halo']} (row {n}), lds {tf['lds']} / {ti['lds']}")
        assert torch.equal(got_f, fwd), (what, want)
        assert torch.equal(got_i, inv), (what, want)
        assert torch.equal(w.inverse(got_f), w.inverse(fwd))
        tile_switch(0)
    hold(host(w.inverse(fwd)), cs["x"], cs["rt_bound"], what + " round trip")


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_forced_resident_where_the_rule_tiles(tile_switch, dt):
    n, levels, key = (12288 if dt == torch.float32 else 6144), 4, "db4"
    cs = case(n, levels, key, dt, 3)
    w = pd.Dwt(key, levels, "cuda:0", dt)
    tf, ti = tile(8, levels, n, dt, False), tile(8, levels, n, dt, True)
    assert tf["resident"] == 0 and ti["resident"] == 0 and tf["tiles"] == ti["tiles"] == 3
    fwd, inv = both(w, cs, dt)
    hold(host(fwd), cs["fwd"], cs["fwd_bound"], f"n {n} {dt} rule (tiled) forward")
    hold(host(inv), cs["inv"], cs["inv_bound"], f"n {n} {dt} rule (tiled) inverse")
    tile_switch(1)
    tf, ti = tile(8, levels, n, dt, False), tile(8, levels, n, dt, True)
    assert (tf["resident"], tf["lds"]) == (1, n * 3 // 2 * EB[dt]) and (ti["resident"], ti["lds"]) == (1, n * 7 // 4 * EB[dt])
    assert 65536 < tf["lds"] < ti["lds"] <= 163840
    got_f, got_i = both(w, cs, dt)
    torch.cuda.synchronize()
    assert torch.equal(got_f, fwd) and torch.equal(got_i, inv)
    # forced resident, the exact in-place call is legal here too
    buf = dev(cs["x"], dt)
    w.forward(buf, out=buf)
    torch.cuda.synchronize()
    assert torch.equal(buf, fwd)
    tile_switch(0)
    # and many tiles on the same row: T capped to 2^J, 768 (f64: 384) tiles, both directions
    tile_switch(2 | ((1 << levels) << 2))
    assert tile(8, levels, n, dt, False)["tiles"] == n >> levels
    got_f, got_i = both(w, cs, dt)
    torch.cuda.synchronize()
    assert torch.equal(got_f, fwd) and torch.equal(got_i, inv)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_refusals_under_the_switch_are_codes_and_launch_nothing(tile_switch, dt):
    w = pd.Dwt("db4", 12, "cuda:0", dt)
    x = torch.zeros((2, 4096), dtype=dt, device="cuda")
    tile_switch(2)
    # the forward depth limit, on a row the resident path would take to any depth
    with pytest.raises(pd.PdspError) as e:
        w.forward(x)
    assert e.value.code == _capi.ERR_UNSUPPORTED_SIZE
    info = (C.c_longlong * 5)()
    assert pd.lib.pdsp_dev_dwt_tile(8, 12, 4096, EB[dt], 0, info) == _capi.ERR_UNSUPPORTED_SIZE
    assert w.max_levels(4096) == 12  # the rule's own answer, whatever the switch says
    # the tiled path shares no bytes, the exact in-place call included
    w3 = pd.Dwt("db4", 3, "cuda:0", dt)
    for run in (w3.forward, w3.inverse):
        with pytest.raises(pd.PdspError) as e:
            run(x, out=x)
        assert e.value.code == _capi.ERR_BAD_ARG
    tile_switch(1)
    big = torch.zeros(1 << 16, dtype=dt, device="cuda")
    with pytest.raises(pd.PdspError) as e:
        w3.forward(big)
    assert e.value.code == _capi.ERR_UNSUPPORTED_SIZE

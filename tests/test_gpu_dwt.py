"""The multi-level wavelet transform on the GPU (pdsp_dwt_kernel.h) against the f64 restatement of the definition in
tests/test_dwt_cpu.py.  Inputs are built in f64 and rounded to the dtype first, the taps are rounded as the handle
rounds them, and the reference is computed in f64 from those rounded values, so the bounds hold the kernels' arithmetic
alone.  With F taps, J levels, eps = 2^-23 (f32) or 2^-52 (f64):

    forward     |got - ref| <= l (F + 2) eps A         for a coefficient of band level l (cD_l; cA_J: l = J),
                                                       A the same recursion with |h|, |g|, |x|
    inverse     |got - ref| <= J (F + 2) eps A'        A' the synthesis of |c| with |h|, |g|
    round trip  |waverec(wavedec(x)) - x| <= J (F + 2) eps S(A + |c_ref|)     S the synthesis with |h|, |g|

Derived, not measured: a level is F fma terms (the inverse: F, two per t), each level's error passes through the next
level's |h|, |g| into the same sum of absolute terms, and eps is twice the unit roundoff; the two spare terms per level
cover the f64 reference's own error and the rounding of the stored value.  Nothing is excluded, and where the abs form
is 0 the output must be exactly 0.  Every case prints its worst share of the bound."""
import functools

import numpy as np
import pytest
import torch

import pragma_dsp_amd as pd
from pragma_dsp_amd import _capi
from test_dwt_cpu import band_levels, lattice_taps, wavedec_ref, waverec_ref

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
EPS = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52}
NP = {torch.float32: np.float32, torch.float64: np.float64}
CUSTOM = {"f6": lattice_taps(6, 61), "f32": lattice_taps(32, 62)}  # orthonormal, not Daubechies: 6 and 32 taps


def wavelet(key):
    """What Dwt() is given: a built-in name, or the taps of a custom filter."""
    return CUSTOM.get(key, key)


def taps(key, dt):
    """The filter as the handle rounds it, in f64."""
    h = CUSTOM[key] if key in CUSTOM else pd.wavelet_taps(key)
    return h.astype(NP[dt]).astype(np.float64)


def signal(shape, dt, seed):
    x = np.random.default_rng(seed).standard_normal(shape)
    return x.astype(NP[dt]).astype(np.float64)


def dev(x, dt):
    return torch.from_numpy(np.array(x)).to(dt).cuda()  # a copy: the shared cases are read-only


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def case(n, levels, key, dt, rows):
    """Inputs and references of one case, computed once and shared (read-only) by every test that needs them."""
    h = taps(key, dt)
    x = signal((rows, n), dt, n + levels)
    c = signal((rows, n), dt, n + levels + 1)
    ref = wavedec_ref(x, h, levels)
    a = wavedec_ref(x, h, levels, abs=True)
    k = levels * (h.size + 2) * EPS[dt]
    out = {
        "h": h, "x": x, "c": c, "fwd": ref, "inv": waverec_ref(c, h, levels),
        "fwd_bound": band_levels(n, levels) * (h.size + 2) * EPS[dt] * a,
        "inv_bound": k * waverec_ref(c, h, levels, abs=True),
        "rt_bound": k * waverec_ref(a + np.abs(ref), h, levels, abs=True),
    }
    for v in out.values():
        v.flags.writeable = False
    return out


def hold(got, ref, bound, what):
    """Every value within its bound, exactly 0 where the bound is 0; prints and returns the worst share."""
    err = np.abs(got - ref)
    pos = bound > 0
    worst = float((err[pos] / bound[pos]).max()) if pos.any() else 0.0
    print(f"{what}: worst |err| / bound = {worst:.3f}")
    assert np.all(got[~pos] == 0.0), what
    assert np.all(err <= bound), (what, worst)
    return worst


# the smallest shapes at which the kernels can go wrong: one pair; filters longer than every level and a last level of
# length 2; a row that is no power of two with a final band of 3; the full decomposition of 4096; every built-in end
# of the table and two custom filters; and rows the rule tiles (12288: one above the resident threshold in f32, 3
# tiles; 98304 = 3 * 2^15 with a halo of 3570; 65536).
CASES = [
    (2, 1, "haar"), (8, 3, "db4"), (8, 3, "f32"), (96, 5, "db2"), (96, 5, "db10"), (96, 5, "f6"),
    (4096, 6, "db1"), (4096, 6, "db2"), (4096, 6, "db4"), (4096, 6, "db10"), (4096, 6, "f6"),
    (4096, 12, "db4"), (4096, 12, "f32"),
    (12288, 4, "db2"), (65536, 4, "db4"), (98304, 8, "db8"), (65536, 10, "haar"),
]
IDS = [f"{n}-{j}-{k}" for n, j, k in CASES]


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n,levels,key", CASES, ids=IDS)
def test_forward_inverse_and_round_trip(n, levels, key, dt):
    rows = 3 + (n + levels) % 3
    cs = case(n, levels, key, dt, rows)
    w = pd.Dwt(wavelet(key), levels, "cuda:0", dt)
    assert (w.levels, w.ntaps) == (levels, cs["h"].size) and w.max_levels(n) >= levels
    what = f"{key} n {n} J {levels} {dt}"
    y = w.forward(dev(cs["x"], dt))
    assert y.shape == (rows, n) and y.dtype == dt
    hold(host(y), cs["fwd"], cs["fwd_bound"], what + " forward")
    hold(host(w.inverse(dev(cs["c"], dt))), cs["inv"], cs["inv_bound"], what + " inverse")
    hold(host(w.inverse(y)), cs["x"], cs["rt_bound"], what + " round trip")


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_zero_rows_and_impulses_are_exact_where_the_abs_form_is_zero(dt):
    # a row of zeros, and an impulse under Haar: most coefficients have A == 0 and must be exactly 0
    n, levels = 64, 4
    x = np.zeros((3, n))
    x[1, 5] = 1.0
    x[2, 63] = -2.5
    h = taps("haar", dt)
    w = pd.Dwt("haar", levels, "cuda:0", dt)
    a = wavedec_ref(x, h, levels, abs=True)
    assert (a == 0).sum() > 2 * n
    y = w.forward(dev(x, dt))
    hold(host(y), wavedec_ref(x, h, levels), band_levels(n, levels) * 4 * EPS[dt] * a, f"impulse {dt}")
    back = host(w.inverse(y))
    assert np.all(back[0] == 0.0)
    hold(back, x, levels * 4 * EPS[dt] * waverec_ref(a + np.abs(wavedec_ref(x, h, levels)), h, levels, abs=True),
         f"impulse round trip {dt}")


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n,levels,key", [(96, 5, "db2"), (4096, 6, "db4"), (12288, 4, "db2")])
def test_strides_offsets_batches_and_guard_bands(n, levels, key, dt):
    """Padded row strides and offset views on both sides; every row's bits are those of the row transformed alone in a
    contiguous buffer; nothing outside the rows is written."""
    rows, pad = 4, 7
    cs = case(n, levels, key, dt, rows)
    w = pd.Dwt(wavelet(key), levels, "cuda:0", dt)
    for direction, src, ref, bound in (("forward", cs["x"], cs["fwd"], cs["fwd_bound"]),
                                       ("inverse", cs["c"], cs["inv"], cs["inv_bound"])):
        run = getattr(w, direction)
        plain = run(dev(src, dt))
        hold(host(plain), ref, bound, f"{key} n {n} {direction} {dt}")
        big = torch.full((rows + 2, n + pad), 7.0, dtype=dt, device="cuda")
        big[1:1 + rows, 3:3 + n] = dev(src, dt)
        out_big = torch.full((rows + 1, n + pad + 2), -3.0, dtype=dt, device="cuda")
        out = out_big[1:, 2:2 + n]
        got = run(big[1:1 + rows, 3:3 + n], out=out)
        assert got is out
        torch.cuda.synchronize()
        assert torch.equal(out, plain)
        guard = out_big.clone()
        guard[1:, 2:2 + n] = -3.0
        assert torch.all(guard == -3.0)
        assert torch.all(big[0] == 7.0) and torch.all(big[:, :3] == 7.0) and torch.all(big[:, 3 + n:] == 7.0)
        for r in (0, rows - 1):
            assert torch.equal(run(dev(src[r:r + 1], dt)), plain[r:r + 1])
        # leading axes flatten into rows
        assert torch.equal(run(dev(src, dt).reshape(2, 2, n)).reshape(rows, n), plain)
        # one-dimensional input: one row
        assert torch.equal(run(dev(src[2], dt)), plain[2])


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n,levels,key", [(2, 1, "haar"), (8, 3, "f32"), (96, 5, "db10"), (4096, 12, "db4")])
def test_exact_in_place_on_the_resident_path(n, levels, key, dt):
    rows = 5
    cs = case(n, levels, key, dt, rows)
    w = pd.Dwt(wavelet(key), levels, "cuda:0", dt)
    for direction, src in (("forward", cs["x"]), ("inverse", cs["c"])):
        run = getattr(w, direction)
        want = run(dev(src, dt))
        buf = dev(src, dt)
        assert run(buf, out=buf) is buf
        torch.cuda.synchronize()
        assert torch.equal(buf, want)
        # with a row stride too
        big = torch.zeros((rows, n + 3), dtype=dt, device="cuda")
        view = big[:, :n]
        view.copy_(dev(src, dt))
        run(view, out=view)
        torch.cuda.synchronize()
        assert torch.equal(view, want) and torch.all(big[:, n:] == 0)


@pytest.mark.parametrize("dt", DTYPES, ids=["f32", "f64"])
def test_refusals_on_the_device_launch_nothing(dt):
    """Codes only: the overlap refusal of the tiled path (the exact in-place call included), overlapping rows on the
    resident path, the forward depth limit on a long row, a wrong dtype."""
    n = 1 << 16
    w = pd.Dwt("db4", 3, "cuda:0", dt)
    x = torch.zeros((2, n), dtype=dt, device="cuda")
    for run in (w.forward, w.inverse):
        with pytest.raises(pd.PdspError) as e:
            run(x, out=x)
        assert e.value.code == _capi.ERR_BAD_ARG and "rows beyond the resident path share no bytes" in str(e.value)
    small = torch.zeros(64 + 32, dtype=dt, device="cuda")
    with pytest.raises(pd.PdspError) as e:
        w.forward(small[:64], out=small[32:])
    assert e.value.code == _capi.ERR_BAD_ARG and "only out == in with equal strides" in str(e.value)
    deep = pd.Dwt("db4", 12, "cuda:0", dt)
    assert deep.max_levels(n) == (10 if dt == torch.float32 else 9) and deep.max_levels(4096) == 12
    with pytest.raises(pd.PdspError) as e:
        deep.forward(x)
    assert e.value.code == _capi.ERR_UNSUPPORTED_SIZE
    with pytest.raises(pd.PdspError) as e:
        w.forward(torch.zeros(100, dtype=dt, device="cuda"))
    assert e.value.code == _capi.ERR_BAD_ARG and str(e.value) == "len must be a positive multiple of 2^levels (levels = 3), got 100"
    other = torch.float64 if dt == torch.float32 else torch.float32
    with pytest.raises(pd.PdspError, match="input must be a"):
        w.forward(torch.zeros(64, dtype=other, device="cuda"))
    with pytest.raises(pd.PdspError, match="out must be a"):
        w.forward(torch.zeros(64, dtype=dt, device="cuda"), out=torch.zeros(32, dtype=dt, device="cuda"))
    assert w.forward(torch.zeros((0, 64), dtype=dt, device="cuda")).shape == (0, 64)


def test_one_shot_split_and_host_forms():
    n, levels, key = 96, 5, "db2"
    cs = case(n, levels, key, torch.float64, 3)
    y = pd.wavedec(dev(cs["x"], torch.float64), key, levels)
    hold(host(y), cs["fwd"], cs["fwd_bound"], "wavedec")
    hold(host(pd.waverec(dev(cs["c"], torch.float64), key, levels)), cs["inv"], cs["inv_bound"], "waverec")
    w = pd.Dwt(key, levels, "cuda:0", torch.float64)
    bands = w.split(y)
    assert [b.shape[-1] for b in bands] == [3, 3, 6, 12, 24, 48] and all(b.data_ptr() >= y.data_ptr() for b in bands)
    assert torch.equal(torch.cat(bands, dim=-1), y)
    # the host forms run the f64 kernels: the same bits
    yh = pd.wavedecHost(cs["x"], key, levels)
    assert yh.dtype == np.float64 and np.array_equal(yh, host(y))
    assert np.array_equal(pd.waverecHost(cs["c"], key, levels), host(pd.waverec(dev(cs["c"], torch.float64), key, levels)))
    assert np.array_equal(pd.wavedecHost(cs["x"][1], key, levels), yh[1])
    assert np.array_equal(pd.wavedecHost(cs["x"].reshape(3, 1, n), key, levels), yh.reshape(3, 1, n))
    # custom taps through the host form, on a row the rule tiles
    big = case(98304, 8, "db8", torch.float64, 3)
    hold(pd.wavedecHost(big["x"], pd.wavelet_taps("db8"), 8), big["fwd"], big["fwd_bound"], "wavedecHost tiled")
    hold(pd.waverecHost(big["c"], pd.wavelet_taps("db8"), 8), big["inv"], big["inv_bound"], "waverecHost tiled")


def test_the_transform_is_ordered_on_the_current_stream():
    """The transform is ordered on the current stream: a forward enqueued behind the copy that fills its input on a side
    stream sees that input."""
    n, levels, key, dt = 4096, 6, "db4", torch.float32
    cs = case(n, levels, key, dt, 4)
    w = pd.Dwt(key, levels, "cuda:0", dt)
    src = torch.from_numpy(cs["x"].astype(np.float32)).pin_memory()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        x = torch.empty((4, n), dtype=dt, device="cuda")
        x.copy_(src, non_blocking=True)
        y = w.forward(x)
    side.synchronize()
    hold(host(y), cs["fwd"], cs["fwd_bound"], "side stream")

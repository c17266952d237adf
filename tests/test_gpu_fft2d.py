"""The 2-D transform (include/pdsp_hip_fft2d.h, pragma_dsp_amd.fft2d) on the card, path by path.

Reference: numpy's f64 fft2 / ifft2 of the inputs after rounding to the dtype.  Metric, per image: max|got - want| /
max|want|.  Bounds: forward and inverse FWD_TOL[dt] * log2(H W) -- the project's forward bound of
tests/test_gpu_stft_pair.py applied at N = H W, because a 2-D pass set is that transform's pass set minus its
twiddles -- and the round trip RT_TOL[dt] * log2(H W) relative to max|x|.  Every case prints an FFT2ERR line with its
ratio to the bound.

The shapes are the smallest at which the code can go wrong: all fifteen resident shapes with a part-filled last
workgroup, every height of the column pass, the narrowest tiles, the widest rows, and a non-square pair in both orders
just past the resident limit.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FWD_TOL = {torch.float32: 8e-8, torch.float64: 2.5e-16}
RT_TOL = {torch.float32: 1e-7, torch.float64: 1.6e-16}
NP = {torch.float32: np.float32, torch.float64: np.float64}
DTYPES = [torch.float32, torch.float64]
IDS = {torch.float32: "f32", torch.float64: "f64"}

RESIDENT = [(1 << a, 1 << b) for a in range(4, 9) for b in range(4, 9) if a + b <= 12]
TWO_PASS = [(h, 512) for h in (16, 32, 64, 128, 256, 512)] + [(512, 16), (512, 32), (256, 32), (128, 64), (64, 128)]
WIDEST = {torch.float32: (16, 16384), torch.float64: (16, 8192)}
BOTH_PATHS = [(32, 64), (128, 64)]  # one resident shape that shares its workgroup (2 images), one two-pass shape

_HANDLES = {}


def handle(h, w):
    import pragma_dsp_amd as pd
    if (h, w) not in _HANDLES:
        _HANDLES[(h, w)] = pd.Fft2d(h, w, DEV)
    return _HANDLES[(h, w)]


def drop_handles():
    """Closes this module's handles (handle() makes them again on demand) and collects the unreachable ones."""
    import gc
    for f in _HANDLES.values():
        f.close()
    _HANDLES.clear()
    gc.collect()


@pytest.fixture(scope="module", autouse=True)
def handles_do_not_outlive_the_module():
    """An Fft2d pins the cached plans of its two lengths while it lives; the modules that count the plan cache down to
    zero (tests/test_gpu_reentrancy.py) must find none of this module's handles left."""
    yield
    drop_handles()


def gauss(seed, shape, dtype, real=False):
    """Gaussian images rounded to the dtype, as complex128 (or float64 when real)."""
    rng = np.random.default_rng(seed)
    re = rng.standard_normal(shape).astype(NP[dtype]).astype(np.float64)
    if real:
        return re
    return re + 1j * rng.standard_normal(shape).astype(NP[dtype]).astype(np.float64)


def planes(x, dtype):
    x = np.asarray(x)
    re = torch.from_numpy(np.ascontiguousarray(x.real).astype(NP[dtype])).to(DEV)
    im = torch.from_numpy(np.ascontiguousarray(x.imag).astype(NP[dtype])).to(DEV) if np.iscomplexobj(x) else None
    return re, im


def as_complex(pair):
    re, im = pair
    torch.cuda.synchronize()
    return re.cpu().numpy().astype(np.float64) + 1j * im.cpu().numpy().astype(np.float64)


def image_err(got, want):
    """max over the images of max|got - want| / max|want|."""
    axes = (-2, -1)
    return float((np.abs(got - want).max(axis=axes) / np.abs(want).max(axis=axes)).max())


def same_bits(a, b):
    return torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int64),
                       b.view(torch.int32 if b.dtype == torch.float32 else torch.int64))


def report(what, dtype, h, w, err, bound):
    print(f"FFT2ERR {what} {IDS[dtype]} {h}x{w} err={err:.3e} bound={bound:.3e} ratio={err / bound:.3f}")


def check_pair(f, x, dtype, what):
    """Forward, inverse and the round trip of the images x against numpy's, each within its bound."""
    h, w = x.shape[-2:]
    lg = math.log2(h * w)
    re, im = planes(x, dtype)
    fwd = f.forward(re, im)
    got = as_complex(fwd)
    e = image_err(got, np.fft.fft2(x))
    report(what + "-fwd", dtype, h, w, e, FWD_TOL[dtype] * lg)
    inv = as_complex(f.inverse(re, im))
    ei = image_err(inv, np.fft.ifft2(x))
    report(what + "-inv", dtype, h, w, ei, FWD_TOL[dtype] * lg)
    back = as_complex(f.inverse(*fwd))
    er = float((np.abs(back - x).max(axis=(-2, -1)) / np.abs(x).max(axis=(-2, -1))).max())
    report(what + "-rt", dtype, h, w, er, RT_TOL[dtype] * lg)
    assert e <= FWD_TOL[dtype] * lg, (h, w, e)
    assert ei <= FWD_TOL[dtype] * lg, (h, w, ei)
    assert er <= RT_TOL[dtype] * lg, (h, w, er)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("shape", RESIDENT, ids=lambda s: f"{s[0]}x{s[1]}")
def test_resident_shapes(shape, dtype):
    h, w = shape
    f = handle(h, w)
    q = f.query(dtype)
    assert q["path"] == "resident" and q["images_per_workgroup"] == 4096 // (h * w) and q["launches"] == 1
    batch = 2 * q["images_per_workgroup"] + 1  # the last workgroup is part-filled
    check_pair(f, gauss(h * 1000 + w, (batch, h, w), dtype), dtype, "resident")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("shape", TWO_PASS + ["widest"], ids=lambda s: s if isinstance(s, str) else f"{s[0]}x{s[1]}")
def test_two_pass_shapes(shape, dtype):
    h, w = WIDEST[dtype] if shape == "widest" else shape
    f = handle(h, w)
    q = f.query(dtype)
    assert q["path"] == "two-pass" and 16 <= q["tile"] <= w and q["launches"] == 2
    check_pair(f, gauss(h * 1000 + w + 1, (3, h, w), dtype), dtype, "twopass")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("shape", [(16, 256), (256, 16), (32, 512), (512, 32)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_orientation(shape, dtype):
    """A unit impulse at (3, 5) gives exp(-2 pi i (3 k / H + 5 l / W)): a swapped or transposed axis misses by O(1)."""
    h, w = shape
    x = np.zeros((2, h, w), dtype=np.complex128)
    x[:, 3, 5] = 1.0
    k, l = np.arange(h)[:, None], np.arange(w)[None, :]
    m = (3 * k * w + 5 * l * h) % (h * w)  # the phase reduced in integers: below one turn, no rounding of a large angle
    want = np.exp(-2j * np.pi * m / (h * w))
    got = as_complex(handle(h, w).forward(*planes(x, dtype)))
    e = image_err(got, np.broadcast_to(want, got.shape))
    report("impulse", dtype, h, w, e, FWD_TOL[dtype] * math.log2(h * w))
    assert e <= FWD_TOL[dtype] * math.log2(h * w)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("shape", BOTH_PATHS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_real_input_is_the_zero_plane_bit_for_bit(shape, dtype):
    h, w = shape
    f = handle(h, w)
    x = gauss(7, (5, h, w), dtype, real=True)
    re, _ = planes(x, dtype)
    a = f.forward(re)
    b = f.forward(re, torch.zeros_like(re))
    torch.cuda.synchronize()
    assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
    e = image_err(as_complex(a), np.fft.fft2(x))
    report("real", dtype, h, w, e, FWD_TOL[dtype] * math.log2(h * w))
    assert e <= FWD_TOL[dtype] * math.log2(h * w)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("shape", [(64, 64), (128, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_norms(shape, dtype):
    h, w = shape
    f = handle(h, w)
    bound = FWD_TOL[dtype] * math.log2(h * w)
    x = gauss(11, (3, h, w), dtype)
    re, im = planes(x, dtype)
    for norm in ("backward", "ortho", "forward", None):
        e = image_err(as_complex(f.forward(re, im, norm=norm)), np.fft.fft2(x, norm=norm))
        ei = image_err(as_complex(f.inverse(re, im, norm=norm)), np.fft.ifft2(x, norm=norm))
        report(f"norm-{norm}", dtype, h, w, max(e, ei), bound)
        assert e <= bound and ei <= bound, (norm, e, ei)
    # forward(x) with norm "forward" = conj-swap identity: the inverse of the swapped planes, norm "backward", swapped back
    a = as_complex(f.forward(re, im, norm="forward"))
    sre, sim = f.inverse(im, re, norm="backward")
    b = as_complex((sim, sre))
    assert image_err(a, b) <= bound


def _expect_bad_arg(call):
    from pragma_dsp_amd import _capi
    with pytest.raises(_capi.PdspError) as ei:
        call()
    assert ei.value.code == _capi.ERR_BAD_ARG, str(ei.value)
    return str(ei.value)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("shape", BOTH_PATHS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_in_place_equals_out_of_place_and_overlaps_are_refused(shape, dtype):
    h, w = shape
    f = handle(h, w)
    batch, n = 5, 5 * h * w
    x = gauss(13, (batch, h, w), dtype)
    re, im = planes(x, dtype)
    want = f.forward(re, im)
    wantr = f.forward(re)
    winv = f.inverse(re, im)
    torch.cuda.synchronize()
    a, b = re.clone(), im.clone()
    got = f.forward(a, b, out=(a, b))
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    a, b = re.clone(), torch.empty_like(re)
    got = f.forward(a, None, out=(a, b))  # a real image in place, its im_out apart
    assert same_bits(got[0], wantr[0]) and same_bits(got[1], wantr[1])
    a, b = re.clone(), im.clone()
    got = f.inverse(a, b, out=(a, b))
    assert same_bits(got[0], winv[0]) and same_bits(got[1], winv[1])

    # every other overlap: refused, outputs untouched.  One buffer, views one image apart (16-byte aligned).
    hw = h * w
    buf = torch.zeros(4 * n + 4 * hw, dtype=dtype, device=DEV)

    def view(off):
        return buf[off:off + n].view(batch, h, w)

    r_in, i_in = view(0), view(2 * n)
    r_in.copy_(re), i_in.copy_(im)
    sentinel = buf.clone()
    apart_r, apart_i = torch.full_like(re, 7.0), torch.full_like(re, 7.0)
    cases = [
        ("re_out one image into re_in", lambda: f.forward(r_in, i_in, out=(view(hw), apart_i))),
        ("im_out one image into im_in", lambda: f.forward(r_in, i_in, out=(apart_r, view(2 * n + hw)))),
        ("re_out is im_in", lambda: f.forward(r_in, i_in, out=(i_in, apart_i))),
        ("im_out is re_in", lambda: f.forward(r_in, i_in, out=(apart_r, r_in))),
        ("planes swapped in place", lambda: f.forward(r_in, i_in, out=(i_in, r_in))),
        ("re in place, im_out moved", lambda: f.forward(r_in, i_in, out=(r_in, apart_i))),
        ("real: im_out is re_in", lambda: f.forward(r_in, None, out=(apart_r, r_in))),
        ("inverse: re_out into im_in", lambda: f.inverse(r_in, i_in, out=(view(2 * n - hw), apart_i))),
        ("outputs overlap each other", lambda: f.forward(r_in, i_in, out=(view(n), view(n + hw)))),
        ("outputs are one tensor", lambda: f.forward(r_in, i_in, out=(apart_r, apart_r))),
    ]
    for name, call in cases:
        msg = _expect_bad_arg(call)
        assert "overlap" in msg, (name, msg)
        torch.cuda.synchronize()
        assert same_bits(buf, sentinel), name
        assert bool((apart_r == 7.0).all()) and bool((apart_i == 7.0).all()), name


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("shape", [(16, 16), (32, 64), (128, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_images_are_independent(shape, dtype):
    h, w = shape
    f = handle(h, w)
    ipw = max(f.query(dtype)["images_per_workgroup"], 1)
    batch = 2 * ipw + 1
    x = gauss(17, (batch, h, w), dtype)
    re, im = planes(x, dtype)
    whole = f.forward(re, im)
    for i in (0, 1, ipw, batch - 1):  # alone, an image takes slot 0 of its workgroup
        one = f.forward(re[i:i + 1].clone(), im[i:i + 1].clone())
        assert same_bits(one[0][0], whole[0][i]) and same_bits(one[1][0], whole[1][i]), i
    j = 1  # on the resident shapes image 1 shares workgroup 0 with image 0
    re2, im2 = re.clone(), im.clone()
    re2[j, h // 2, w // 3] = float("nan")
    sick = f.forward(re2, im2)
    torch.cuda.synchronize()
    keep = [i for i in range(batch) if i != j]
    assert same_bits(sick[0][keep], whole[0][keep]) and same_bits(sick[1][keep], whole[1][keep])
    assert bool(torch.isnan(sick[0][j]).any())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
def test_stream_entry_points_refuse_bad_arguments(dtype):
    """The checks of pdsp_fft2d_c2c_* behind the handle, in their order, with their texts; nothing is launched."""
    from pragma_dsp_amd import _capi
    f = handle(32, 64)
    fn = getattr(_capi.lib, "pdsp_fft2d_c2c_" + IDS[dtype])
    re, im = planes(gauss(3, (2, 32, 64), dtype), dtype)
    ore, oim = torch.full_like(re, 7.0), torch.full_like(re, 7.0)
    p = [t.data_ptr() for t in (re, im, ore, oim)]

    def refused(batch, a, b, c, d, inverse, norm, text):
        assert fn(f._h, batch, a, b, c, d, inverse, norm, None) == _capi.ERR_BAD_ARG
        assert _capi.lib.pdsp_last_error().decode() == text

    refused(0, *p, 0, 0, "batch must be >= 1, got 0")
    refused(2, *p, 0, 3, "2-D FFT norm must be 0 (backward), 1 (ortho) or 2 (forward), got 3")
    refused(2, None, p[1], p[2], p[3], 0, 0, "null buffer")
    refused(2, p[0], p[1], None, p[3], 0, 0, "null buffer")
    refused(2, p[0], p[1], p[2], None, 0, 0, "null buffer")
    refused(2, p[0], None, p[2], p[3], 1, 0, "the inverse needs both planes (im_in is null)")
    refused(2, p[0] + re.element_size(), p[1], p[2], p[3], 0, 0, "the planes must begin on 16-byte boundaries")
    torch.cuda.synchronize()
    assert bool((ore == 7.0).all()) and bool((oim == 7.0).all())
    if dtype == torch.float64:  # a shape of the f32 domain alone: the handle exists, the f64 call is refused
        import pragma_dsp_amd as pd
        wide = pd.Fft2d(16, 16384, DEV)
        assert wide.query(torch.float32)["path"] == "two-pass"
        x = torch.zeros((1, 16, 16384), dtype=dtype, device=DEV)
        with pytest.raises(_capi.PdspError) as ei:
            wide.forward(x, x.clone())
        assert ei.value.code == _capi.ERR_UNSUPPORTED_SIZE and "8192 in f64" in str(ei.value)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("shape", BOTH_PATHS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_guard_bands_stay_intact(shape, dtype):
    h, w = shape
    f = handle(h, w)
    batch, guard = 3, 64
    n = batch * h * w
    re, im = planes(gauss(19, (batch, h, w), dtype), dtype)
    bufs = [torch.full((guard + n + guard,), float("nan"), dtype=dtype, device=DEV) for _ in range(2)]
    outs = tuple(b[guard:guard + n].view(batch, h, w) for b in bufs)
    got = f.forward(re, im, out=outs)
    want = f.forward(re, im)
    torch.cuda.synchronize()
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    for b in bufs:
        assert bool(torch.isnan(b[:guard]).all()) and bool(torch.isnan(b[guard + n:]).all())
        assert not bool(torch.isnan(b[guard:guard + n]).any())


@pytest.mark.parametrize("shape,dtype", [((64, 64), torch.float32), ((16, 16), torch.float64), ((128, 64), torch.float32)],
                         ids=["64x64-f32", "16x16-f64", "128x64-f32"])
def test_machine_filling_batch_equals_batches_of_seven(shape, dtype):
    from pragma_dsp_amd import _capi
    h, w = shape
    f = handle(h, w)
    q = f.query(dtype)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # workgroups per image of the launch with the fewest: 1 / images on the resident path; on the two-pass path the
    # staged row kernel takes 4096 points and the column kernel `tile` columns per workgroup
    per_image = 1.0 / q["images_per_workgroup"] if q["path"] == "resident" else min(h * w // 4096, w // q["tile"])
    batch = math.ceil(32 * cus / per_image)
    assert batch * per_image >= 32 * cus
    gen = torch.Generator(device=DEV).manual_seed(23)
    re = torch.randn((batch, h, w), dtype=dtype, device=DEV, generator=gen)
    im = torch.randn((batch, h, w), dtype=dtype, device=DEV, generator=gen)
    whole = f.forward(re, im)
    pre, pim = torch.empty_like(re), torch.empty_like(re)
    fn = getattr(_capi.lib, "pdsp_fft2d_c2c_" + IDS[dtype])
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    step = h * w * re.element_size()
    for i in range(0, batch, 7):
        nb, off = min(7, batch - i), i * step
        rc = fn(f._h, nb, re.data_ptr() + off, im.data_ptr() + off, pre.data_ptr() + off, pim.data_ptr() + off, 0, 0,
                stream)
        assert rc == 0, _capi.lib.pdsp_last_error()
    torch.cuda.synchronize()
    assert same_bits(whole[0], pre) and same_bits(whole[1], pim)
    x = (re[-2:].cpu().numpy().astype(np.float64) + 1j * im[-2:].cpu().numpy().astype(np.float64))
    e = image_err(as_complex((whole[0][-2:], whole[1][-2:])), np.fft.fft2(x))
    report("filling", dtype, h, w, e, FWD_TOL[dtype] * math.log2(h * w))
    assert e <= FWD_TOL[dtype] * math.log2(h * w)


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("lead", [(), (2, 3)], ids=["HW", "23HW"])
@pytest.mark.parametrize("shape", [(64, 64), (128, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_host_forms(shape, lead, real):
    import pragma_dsp_amd as pd
    h, w = shape
    bound = FWD_TOL[torch.float64] * math.log2(h * w)
    x = gauss(29, lead + (h, w), torch.float64, real=real)
    got = pd.fft2(x)
    assert got.dtype == np.complex128 and got.shape == x.shape
    e = image_err(got, np.fft.fft2(x))
    ei = image_err(pd.ifft2(x), np.fft.ifft2(x))
    eo = image_err(pd.fft2(x, norm="ortho"), np.fft.fft2(x, norm="ortho"))
    report("host", torch.float64, h, w, max(e, ei, eo), bound)
    assert e <= bound and ei <= bound and eo <= bound, (e, ei, eo)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS.get)
@pytest.mark.parametrize("shape", BOTH_PATHS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_graph_capture_and_replay(shape, dtype):
    """Both c2c entry points, captured on a side stream with the handle made beforehand and no call before the capture:
    every table was uploaded at create.  The plans are cold: this module's handles are closed and the plan cache is
    emptied first, so create makes both plans anew and a table left to the first call would have to go up inside the
    capture."""
    import pragma_dsp_amd as pd
    from pragma_dsp_amd import _capi
    h, w = shape
    drop_handles()
    assert pd.lib.pdsp_plan_cache_clear() == 0
    before = _capi.live_resources()
    assert before["cached_plans"] == before["pinned"]  # nothing unpinned is left: the clear took it
    f = pd.Fft2d(h, w, DEV)  # a fresh handle on fresh plans: its first call is the captured one
    made = _capi.live_resources()
    assert made["cached_plans"] == before["cached_plans"] + 2 and made["tables"] > before["tables"]
    xa, xb = gauss(31, (5, h, w), dtype), gauss(37, (5, h, w), dtype)
    re, im = planes(xa, dtype)
    ore, oim = torch.full_like(re, float("nan")), torch.full_like(re, float("nan"))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.graph(g, stream=side):
        f.forward(re, im, out=(ore, oim))
    torch.cuda.synchronize()
    assert bool(torch.isnan(ore).all()) and bool(torch.isnan(oim).all()), "work ran during the capture"
    assert _capi.live_resources() == made, "the capture uploaded, allocated or created something"
    for x in (xa, xb):
        nre, nim = planes(x, dtype)
        re.copy_(nre), im.copy_(nim)
        eager = f.forward(re, im)
        torch.cuda.synchronize()
        for _ in range(2):
            ore.fill_(float("nan")), oim.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert same_bits(ore, eager[0]) and same_bits(oim, eager[1])
    del g


def test_a_handle_pins_its_two_plans_and_releases_them():
    """The object borrows the cached plans of W and H points: pinned while it lives (pdsp_plan_cache_clear leaves them
    and the handle keeps working), released when it is destroyed."""
    import pragma_dsp_amd as pd
    from pragma_dsp_amd import _capi
    drop_handles()
    assert pd.lib.pdsp_plan_cache_clear() == 0
    start = _capi.live_resources()  # whatever another module still holds stays in every count below
    assert start["cached_plans"] == start["pinned"]
    f = pd.Fft2d(512, 2048, DEV)  # lengths no other handle of the suite is likely to hold
    re, im = planes(gauss(41, (1, 512, 2048), torch.float32), torch.float32)
    want = f.forward(re, im)
    torch.cuda.synchronize()
    assert pd.lib.pdsp_plan_cache_clear() == 0
    live = _capi.live_resources()
    assert live["pinned"] == start["pinned"] + 2 and live["cached_plans"] == start["cached_plans"] + 2
    got = f.forward(re, im)
    torch.cuda.synchronize()
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    f.close()
    assert _capi.live_resources()["pinned"] == start["pinned"]
    assert pd.lib.pdsp_plan_cache_clear() == 0
    assert _capi.live_resources() == start

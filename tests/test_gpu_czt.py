"""The chirp-z transform on the device (pdsp_czt_kernel.h: Czt.forward, pdsp_czt_f32 / _f64, czt / zoom_fft) against
a direct sum with EXACT phases on the same inputs (Gaussian complex rows rounded to the dtype first), f32 and f64.

Reference (tests/test_czt_cpu.py: grid_direct): the grid cases use step = p / 2^20 and start = q / 2^20, so the phase
index n k p + n q reduces mod 2^20 in int64; cos / sin come from one long double table; the K columns are evaluated in
chunks; the f64 reference accumulates in long double.  At M = 8192 three rows (first, middle, last of the 37) are
referenced.

Metric per row: e = max_k |got - want| / max(max_k |want|, ||x radius^-n||_2); the norm term keeps a row of one or two
bins from dividing by a chance-small value.

Bound: RT_TOL[dt] * log2 M + 4 eps(dt), M the points of the circular convolution -- the any-length DFT's bound
(tests/test_gpu_dft.py), unchanged: RT_TOL * log2 M is the project's bound for a forward plus an inverse pass set of M
points, the 4 eps are for the two chirp multiplications and the rounded tables.  The same algorithm emulated on the CPU
at complex64 / complex128 stays at or below 0.53 of it.

Every case prints a `CZTERR` line with what it measured."""
import ctypes as C
import math

import numpy as np
import pytest

from test_czt_cpu import GRID, LD, PI, cis, conv_size, grid_direct, grid_table, row_err, turns
from test_gpu_dft import (EPS, ROWS, RT_TOL, SENTINEL, _t, cplx, gauss, padding_untouched, rows_per_wg, same_bits,
                          strided)

pytestmark = pytest.mark.gpu

DTS = ["f32", "f64"]
P, Q = 401, 123457  # the grid cases' step = P / 2^20 (a band of ~0.4 K / 1024 turns) and start = Q / 2^20


def ends():
    """Both ends of every M: L + K - 1 = M (every slot of b is used) and = M / 2 + 1, each once with K < L and once
    with K > L."""
    out = []
    for log2m in range(5, 14):
        m = 1 << log2m
        for total in (m + 1, m // 2 + 2):  # L + K
            small = total // 3
            out += [(total - small, small), (small, total - small)]
    return out


ENDS = ends()
STRETCHED = [(1, 7), (4096, 1), (8191, 2), (500, 3000)]


def bound(dt, ln, bins):
    return RT_TOL[dt] * (conv_size(ln, bins).bit_length() - 1) + 4 * EPS[dt]


_czts = {}


def czt_of(ln, bins, step, start=0.0, radius=1.0):
    import pragma_dsp_amd as pd
    key = (ln, bins, step, start, radius)
    if key not in _czts:
        c = _czts[key] = pd.Czt(ln, bins, step, start, radius)
        assert (c.length, c.bins, c.conv_size) == (ln, bins, conv_size(ln, bins))
    return _czts[key]


_refs = {}


def reference(z, bins, p, q, radius, dt, key):
    """grid_direct of the rows the case references, computed once per case."""
    if key not in _refs:
        rows = [0, ROWS // 2, ROWS - 1] if conv_size(z.shape[-1], bins) == 8192 and len(z) == ROWS else list(range(len(z)))
        _refs[key] = (rows, grid_direct(z[rows], bins, p, q, radius, extended=(dt == "f64")))
    return _refs[key]


def grid_case(ln, bins, dt, radius=1.0, what="grid"):
    c = czt_of(ln, bins, P / GRID, Q / GRID, radius)
    re, im, z = gauss(1000 * ln + 2 * bins + (dt == "f64"), ROWS, ln, dt)
    got = cplx(c.forward(re, im))
    assert got.shape == (ROWS, bins)
    rows, want = reference(z, bins, P, Q, radius, dt, (ln, bins, radius, dt))
    e = row_err(got[rows], want, z[rows], radius)
    b = bound(dt, ln, bins)
    print(f"CZTERR {what} {dt} L={ln} K={bins} M={c.conv_size} radius={radius} e={e:.3e} bound={b:.3e} share={e / b:.2f}")
    assert e <= b


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ln,bins", ENDS)
def test_both_ends_of_every_m(ln, bins, dt):
    m = conv_size(ln, bins)
    assert ln + bins - 1 in (m, m // 2 + 1) and (rows_per_wg(m) == 1 or ROWS % rows_per_wg(m))
    grid_case(ln, bins, dt, what="end")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ln,bins", STRETCHED)
def test_degenerate_and_stretched_shapes(ln, bins, dt):
    grid_case(ln, bins, dt, what="stretched")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("radius", [0.999, 1.001])
def test_radius(radius, dt):
    grid_case(1000, 1000, dt, radius=radius, what="radius")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ln,bins", [(3, 5), (17, 40), (1000, 700), (4095, 1000)])
def test_unit_impulses(ln, bins, dt):
    """An impulse at p gives radius^-p exp(-2 pi i (p k step + p start))."""
    import torch
    step, start, radius = 0.37 / bins, 0.123, 0.9995
    c = czt_of(ln, bins, step, start, radius)
    ps = sorted({0, 1, ln - 1})
    re = torch.zeros((len(ps), ln), dtype=_t(dt), device="cuda")
    for r, p in enumerate(ps):
        re[r, p] = 1.0
    k = np.arange(bins, dtype=np.int64)
    want = np.stack([radius ** -float(p) * cis(-(turns(p * k, step, 1.0) + turns(p, start, 1.0))) for p in ps])
    x = re.double().cpu().numpy()
    for got in (c.forward(re), c.forward(re, torch.zeros_like(re))):
        e = row_err(cplx(got), want, x, radius)
        print(f"CZTERR impulse {dt} L={ln} K={bins} e={e:.3e} bound={bound(dt, ln, bins):.3e}")
        assert e <= bound(dt, ln, bins)


def dirichlet(ln, j):
    """sum_{n < L} exp(-2 pi i n j / 2^20), j integers: exp(-pi i (L - 1) d) sin(pi L d) / sin(pi d), d = j / 2^20,
    with every angle reduced in integers."""
    j = np.asarray(j, dtype=np.int64) % GRID
    d = PI * j.astype(LD) / GRID
    num = np.sin(PI * ((ln * j) % (2 * GRID)).astype(LD) / GRID)
    den = np.sin(d)
    mag = np.where(j == 0, LD(ln), num / np.where(j == 0, LD(1), den)).astype(np.float64)
    return mag * cis(-(((ln - 1) * j) % (2 * GRID)).astype(LD) / (2 * GRID))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ln,bins", [(100, 37), (1000, 256), (4096, 256)])
def test_a_tone_on_a_zoom_bin(ln, bins, dt):
    """A tone exactly on zoom bin k0 peaks there with value L; every other bin holds the Dirichlet kernel's value."""
    import torch
    c = czt_of(ln, bins, P / GRID, Q / GRID)
    k0s = [0, 1, bins // 2, bins - 1]
    n = np.arange(ln, dtype=np.int64)
    cs, sn = grid_table()
    idx = np.stack([(n * ((Q + k0 * P) % GRID)) % GRID for k0 in k0s])
    re, im = (torch.from_numpy(p.astype(np.float64)).to(_t(dt)).cuda() for p in (cs[idx], -sn[idx]))
    got = cplx(c.forward(re, im))
    k = np.arange(bins, dtype=np.int64)
    b = bound(dt, ln, bins)
    for r, k0 in enumerate(k0s):
        want = dirichlet(ln, (k - k0) * P)
        assert want[k0] == ln and int(np.abs(got[r]).argmax()) == k0
        peak = abs(got[r, k0] - ln) / ln
        rest = np.abs(np.delete(got[r] - want, k0)).max() / ln
        print(f"CZTERR tone {dt} L={ln} K={bins} k0={k0} peak={peak:.3e} rest={rest:.3e} bound={b:.3e}")
        assert peak <= b and rest <= b


@pytest.mark.parametrize("dt,ln", [("f64", 1024), ("f32", 1000)])
def test_the_dft_against_numpy(dt, ln):
    """Czt(L, L, 1 / L) is the DFT: in f64 at L = 1024, where 1 / L is exact; in f32 at L = 1000, where the rounding of
    1 / L (1e-11 rad at the far corner) is invisible."""
    c = czt_of(ln, ln, 1.0 / ln)
    re, im, z = gauss(ln, ROWS, ln, dt)
    e = row_err(cplx(c.forward(re, im)), np.fft.fft(z), z)
    print(f"CZTERR dft {dt} L={ln} e={e:.3e} bound={bound(dt, ln, ln):.3e}")
    assert e <= bound(dt, ln, ln)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ln,fn,bins,pad", [(1000, [0, 2], 2048, 2048), (300, [0, 2], 512, 512), (1000, [0, 0.5], 512, 2048),
                                            (100, 1.0, 64, 128)])
def test_zoom_against_a_padded_fft(ln, fn, bins, pad, dt):
    """Czt.zoom on a band whose step is dyadic: the first `bins` bins of numpy.fft.fft of the row zero-padded to `pad`."""
    import pragma_dsp_amd as pd
    c = pd.Czt.zoom(ln, fn, bins, fs=2)
    assert c.step == 1.0 / pad and c.start == 0.0 and (c.length, c.bins) == (ln, bins)
    re, im, z = gauss(ln + bins, ROWS, ln, dt)
    e = row_err(cplx(c.forward(re, im)), np.fft.fft(z, pad)[:, :bins], z)
    print(f"CZTERR zoom {dt} L={ln} K={bins} pad={pad} e={e:.3e} bound={bound(dt, ln, bins):.3e}")
    assert e <= bound(dt, ln, bins)


BITS = [(1, 7), (17, 40), (40, 17), (1000, 700), (700, 1000), (4096, 256)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ln,bins", BITS)
def test_real_input_is_the_complex_call_with_a_zero_plane(ln, bins, dt):
    import torch
    c = czt_of(ln, bins, P / GRID, Q / GRID)
    re, _, _ = gauss(ln + bins, ROWS, ln, dt)
    assert same_bits(c.forward(re), c.forward(re, torch.zeros_like(re)))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ln,bins", BITS)
def test_a_row_does_not_depend_on_its_batch_or_its_strides(ln, bins, dt):
    """Two calls, rows at strides L + 7 in and K + 5 out from bases one element into their allocations (so rows are
    misaligned for anything wider than an element), and rows run alone, all give the bits of the contiguous batch.  The
    input rows are followed by NaN up to their stride and the output rows lie in NaN: every output is finite and every
    sentinel is untouched."""
    c = czt_of(ln, bins, P / GRID, Q / GRID)
    re, im, _ = gauss(3 * ln + bins, ROWS, ln, dt)
    full = c.forward(re, im)
    assert same_bits(full, c.forward(re, im))
    ins = [strided(ROWS, ln, ln + 7, dt, offset=1) for _ in range(2)]
    outs = [strided(ROWS, bins, bins + 5, dt, offset=1) for _ in range(2)]
    ins[0][1].copy_(re)
    ins[1][1].copy_(im)
    got = c.forward(ins[0][1], ins[1][1], out=(outs[0][1], outs[1][1]))
    assert got[0].data_ptr() == outs[0][1].data_ptr() and got[1].data_ptr() == outs[1][1].data_ptr()
    assert all(padding_untouched(b, v) for b, v in ins + outs)  # (and no NaN inside the views)
    assert same_bits(got, full)
    assert same_bits((ins[0][1], ins[1][1]), (re, im))  # the inputs are read only
    for r in (0, 17, ROWS - 1):
        alone = c.forward(re[r:r + 1].clone(), im[r:r + 1].clone())
        assert same_bits(alone, (full[0][r:r + 1], full[1][r:r + 1])), r
    # one row more than a workgroup holds: the last workgroup's other rows are dead
    rows = rows_per_wg(c.conv_size) + 1
    part = c.forward(re[:rows].clone(), im[:rows].clone()) if rows <= ROWS else None
    assert part is None or same_bits(part, (full[0][:rows], full[1][:rows]))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ln,bins", [(17, 40), (40, 17), (1000, 700), (700, 1000), (4096, 256), (97, 97)])
def test_exact_in_place(ln, bins, dt):
    """re_out == re_in, im_out == im_in at one stride >= max(L, K) gives the out-of-place bits, for K < L and K > L;
    a real row takes an im_out of its own."""
    import torch
    c = czt_of(ln, bins, P / GRID, Q / GRID)
    re, im, _ = gauss(5 * ln + bins, ROWS, ln, dt)
    want, want_real = c.forward(re, im), c.forward(re)
    stride = max(ln, bins) + 3
    bufs = [torch.zeros((ROWS * stride + 9,), dtype=_t(dt), device="cuda") for _ in range(3)]
    vin = [b.as_strided((ROWS, ln), (stride, 1), 1) for b in bufs]
    vout = [b.as_strided((ROWS, bins), (stride, 1), 1) for b in bufs]
    vin[0].copy_(re)
    vin[1].copy_(im)
    assert same_bits(c.forward(vin[0], vin[1], out=(vout[0], vout[1])), want)
    vin[0].copy_(re)
    assert same_bits(c.forward(vin[0], None, out=(vout[0], vout[2])), want_real)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ln,bins", [(97, 40), (40, 97)])
def test_other_overlaps_and_short_strides_are_refused(ln, bins, dt):
    import torch
    from pragma_dsp_amd import _capi, lib
    rows = 5
    big, small = max(ln, bins), min(ln, bins)
    c = czt_of(ln, bins, P / GRID, Q / GRID)
    fn = lib.pdsp_czt_f32 if dt == "f32" else lib.pdsp_czt_f64
    es = 4 if dt == "f32" else 8
    re = torch.full(((rows + 2) * big,), 1.0, dtype=_t(dt), device="cuda")
    im = torch.full(((rows + 2) * big,), 2.0, dtype=_t(dt), device="cuda")
    o1 = torch.full(((rows + 1) * big,), SENTINEL, dtype=_t(dt), device="cuda")
    o2 = torch.full(((rows + 1) * big,), SENTINEL, dtype=_t(dt), device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off * es)  # noqa: E731

    def refused(re_in, im_in, re_out, im_out, in_stride=big, out_stride=big, text=b"output overlaps input"):
        assert fn(c._h, rows, re_in, im_in, in_stride, re_out, im_out, out_stride, None) == _capi.ERR_BAD_ARG
        assert lib.pdsp_last_error().startswith(text), lib.pdsp_last_error()

    refused(p(re), p(im), p(re, big), p(im, big))      # both outputs one row down their inputs
    refused(p(re), p(im), p(re, big), p(o2))           # one of them
    refused(p(re), p(im), p(o1), p(im, 1))             # one element
    refused(p(re), p(im), p(im), p(o2))                # re_out == im_in
    refused(p(re), p(im), p(im), p(re))                # the planes exchanged
    refused(p(re), p(im), p(re), p(o2))                # complex rows in place in one plane only
    refused(p(re), p(im), p(re), p(im), big, big + 1)  # the same bases at different strides
    refused(p(re), p(im), p(re), p(im), ln, bins)      # ... the tight stride of each side
    refused(p(re), None, p(re), p(re, 1))              # a real row in place whose im_out meets the samples
    # in place, with the imaginary plane one element past the shorter side's extent of the real one: it lies inside
    # the longer side's
    refused(p(re), p(re, (rows - 1) * big + small), p(re), p(re, (rows - 1) * big + small))
    refused(p(re), p(im), p(o1), p(o1), text=b"the output planes overlap")  # im_out == re_out
    refused(p(re), p(im), p(o1), p(o1, 1), text=b"the output planes overlap")
    torch.cuda.synchronize()
    assert bool((re == 1.0).all()) and bool((im == 2.0).all())
    assert bool(torch.isnan(o1).all()) and bool(torch.isnan(o2).all())
    # the other checks, ahead of any device work as well
    short = b"strides must be >= L = %d in and >= K = %d out" % (ln, bins)
    for args, text in (((0, p(re), p(im), big, p(o1), p(o2), big), b"batch must be >= 1, got 0"),
                       ((rows, p(re), p(im), ln - 1, p(o1), p(o2), big), short),
                       ((rows, p(re), p(im), big, p(o1), p(o2), bins - 1), short),
                       ((rows, None, p(im), big, p(o1), p(o2), big), b"null buffer"),
                       ((rows, p(re), p(im), big, None, p(o2), big), b"null buffer"),
                       ((rows, p(re), p(im), big, p(o1), None, big), b"null buffer"),
                       ((1 << 31, p(re), p(im), big, p(o1), p(o2), big), b"batch too large"),
                       ((1 << 40, p(re), p(im), 1 << 40, p(o1), p(o2), big), b"batch 1099511627776 x stride overflows")):
        assert fn(c._h, *args, None) == _capi.ERR_BAD_ARG
        assert lib.pdsp_last_error().startswith(text), lib.pdsp_last_error()
    torch.cuda.synchronize()
    assert bool((re == 1.0).all()) and bool((im == 2.0).all())
    assert bool(torch.isnan(o1).all()) and bool(torch.isnan(o2).all())


def test_python_form_refuses_planes_of_other_shapes():
    import torch
    import pragma_dsp_amd as pd
    c = czt_of(100, 37, P / GRID, Q / GRID)
    re = torch.zeros((4, 100), device="cuda")
    for bad in (lambda: c.forward(re[:, :99]), lambda: c.forward(re, re.double()), lambda: c.forward(re, re[:3]),
                lambda: c.forward(re, out=(re, re)), lambda: c.forward(re, out=(torch.zeros((4, 37), device="cuda"),)),
                lambda: c.forward(re.cpu()), lambda: c.forward(re.t())):
        with pytest.raises(pd.PdspError):
            bad()
    out = c.forward(re.reshape(2, 2, 100))
    assert out[0].shape == (2, 2, 37) and not out[0].any() and not out[1].any()  # zeros give exact zeros


def test_host_forms_against_the_direct_sum():
    import torch
    import pragma_dsp_amd as pd
    rng = np.random.default_rng(5)
    for ln, bins in ((1, 4), (300, 512), (1000, 256), (3000, 1024)):
        z = rng.standard_normal((3, ln)) + 1j * rng.standard_normal((3, ln))
        b = bound("f64", ln, bins)
        # czt: w = None is step = 1 / m, dyadic here; a = 0.9995 i is radius 0.9995 at a quarter turn
        radius = 0.9995 if ln <= 1000 else 1.0
        got = pd.czt(z, bins, a=radius * 1j)
        assert got.dtype == np.complex128 and got.shape == (3, bins)
        ec = row_err(got, grid_direct(z, bins, GRID // bins, GRID // 4, radius), z, radius)
        er = row_err(pd.czt(z.real, bins), grid_direct(z.real, bins, GRID // bins), z.real)
        # zoom_fft: the band [0.25, 0.75) of fs = 2 in `bins` points is step = 1 / (4 bins), start = 1 / 8
        ez = row_err(pd.zoom_fft(z, [0.25, 0.75], bins), grid_direct(z, bins, GRID // (4 * bins), GRID // 8), z)
        e1 = row_err(pd.zoom_fft(z[0], 0.5, bins), grid_direct(z[:1], bins, GRID // (4 * bins))[0], z[0])  # 1-D, scalar fn
        print(f"CZTERR host f64 L={ln} K={bins} czt={ec:.3e} real={er:.3e} zoom={ez:.3e} 1d={e1:.3e} bound={b:.3e}")
        assert max(ec, er, ez, e1) <= b
    # m defaults to the length (L = K = 1024: the DFT, 1 / 1024 exact)
    x = rng.standard_normal(1024)
    assert row_err(pd.czt(x), np.fft.fft(x), x) <= bound("f64", 1024, 1024)
    # the host form is the f64 device form, also for a complex w, whose angle becomes step
    w, a = complex(np.exp(-2j * np.pi * 0.37 / 700)), complex(0.9995 * np.exp(0.3j))
    step, start = -math.atan2(w.imag, w.real) / (2 * math.pi), math.atan2(a.imag, a.real) / (2 * math.pi)
    dev = czt_of(1024, 700, step, start, abs(a)).forward(torch.from_numpy(x[None]).cuda())
    assert np.array_equal(cplx(dev)[0], pd.czt(x, 700, w, a))

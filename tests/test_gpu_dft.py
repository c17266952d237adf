"""The any-length DFT on the device (pdsp_bluestein_kernel.h: Dft.forward / .inverse, pdsp_dft_c2c_*, dft / idft)
against numpy.fft.fft / ifft in f64 on the same inputs (rounded to the dtype first), f32 and f64.

Metric per row: e = max|got - want| / max|want|.

Bound: RT_TOL[dt] * log2 M + 4 eps(dt), M the points of the circular convolution.  RT_TOL * log2 M is the project's
own bound for a forward plus an inverse pass set of M points (tests/test_gpu_stft_pair.py, tests/test_gpu_hilbert.py):
1e-7 in f32, 1.6e-16 in f64; the 4 eps are for the two chirp multiplications and the rounded chirp and filter tables.
The same algorithm emulated on the CPU at complex64 / complex128 stays at or below 0.51 of it for every length here.

Lengths: both ends of every M = 32 ... 8192 -- the largest L is M / 2, the smallest M / 4 + 1 (L = 2 for M = 32), where
a wrong M or a wrong layout of the chirp filter aliases the circular convolution -- and 3, 5, 17, 97, 1000, 1023, 4095.
Every case prints a `DFTERR` line with what it measured."""
import ctypes as C

import numpy as np
import pytest

from test_dft_cpu import conv_size, row_err

pytestmark = pytest.mark.gpu

RT_TOL = {"f32": 1e-7, "f64": 1.6e-16}  # x log2 M (tests/test_gpu_stft_pair.py)
EPS = {"f32": 2.0 ** -23, "f64": 2.0 ** -52}
SENTINEL = float("nan")
ROWS = 37
ENDS = sorted({2} | {m // 2 for m in (1 << l for l in range(5, 14))} | {m // 4 + 1 for m in (1 << l for l in range(6, 14))})
LENGTHS = sorted(set(ENDS) | {3, 5, 17, 97, 1000, 1023, 4095})
DTS = ["f32", "f64"]


def bound(dt, ln):
    return RT_TOL[dt] * (conv_size(ln).bit_length() - 1) + 4 * EPS[dt]


def rows_per_wg(m):
    tp = m // 16
    return max(tp, 256) // tp


def _t(dt):
    import torch
    return torch.float32 if dt == "f32" else torch.float64


_dfts = {}


def dft_of(ln):
    import pragma_dsp_amd as pd
    if ln not in _dfts:
        _dfts[ln] = pd.Dft(ln)
        assert _dfts[ln].length == ln and _dfts[ln].conv_size == conv_size(ln)
    return _dfts[ln]


def gauss(seed, rows, ln, dt):
    """Gaussian complex rows rounded to the dtype: (re, im) on the device and the same values as complex128."""
    import torch
    rng = np.random.default_rng(seed)
    re = torch.from_numpy(rng.standard_normal((rows, ln))).to(_t(dt))
    im = torch.from_numpy(rng.standard_normal((rows, ln))).to(_t(dt))
    return re.cuda(), im.cuda(), re.double().numpy() + 1j * im.double().numpy()


def cplx(pair):
    return pair[0].double().cpu().numpy() + 1j * pair[1].double().cpu().numpy()


def strided(rows, ln, stride, dt, offset=0, fill=SENTINEL):
    """A [rows, ln] view at row stride `stride`, `offset` elements into a buffer filled with `fill`."""
    import torch
    buf = torch.full((offset + rows * stride + 8,), fill, dtype=_t(dt), device="cuda")
    return buf, buf.as_strided((rows, ln), (stride, 1), offset)


def padding_untouched(buf, view):
    """Every element of buf outside the view still holds the NaN sentinel."""
    import torch
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(False)
    return bool(torch.isnan(buf[mask]).all()) and not bool(torch.isnan(view).any())


def bits(pair):
    return [p.cpu().numpy().view(np.uint32 if p.element_size() == 4 else np.uint64) for p in pair]


def same_bits(a, b):
    return all(np.array_equal(x, y) for x, y in zip(bits(a), bits(b)))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ln", LENGTHS)
def test_forward_and_inverse_against_numpy(ln, dt):
    d = dft_of(ln)
    re, im, z = gauss(1000 * ln + (dt == "f64"), ROWS, ln, dt)
    ef = row_err(cplx(d.forward(re, im)), np.fft.fft(z))
    ei = row_err(cplx(d.inverse(re, im)), np.fft.ifft(z))
    print(f"DFTERR {dt} L={ln} M={d.conv_size} fwd={ef:.3e} inv={ei:.3e} bound={bound(dt, ln):.3e}")
    assert ef <= bound(dt, ln) and ei <= bound(dt, ln)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ln", [2, 17, 1000, 4095, 4096])
def test_real_input_is_the_complex_call_with_a_zero_plane(ln, dt):
    import torch
    d = dft_of(ln)
    re, _, z = gauss(ln, ROWS, ln, dt)
    got = d.forward(re)
    assert same_bits(got, d.forward(re, torch.zeros_like(re)))
    assert row_err(cplx(got), np.fft.fft(z.real)) <= bound(dt, ln)


def _twiddle(num, ln):
    """exp(-2 pi i num / L) with num reduced mod L in integers."""
    return np.exp(-2j * np.pi * (np.asarray(num, dtype=np.int64) % ln).astype(np.float64) / ln)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ln", [3, 17, 1000, 4095])
def test_unit_impulses(ln, dt):
    import torch
    d = dft_of(ln)
    ps = [0, 1, ln - 1]
    re = torch.zeros((len(ps), ln), dtype=_t(dt), device="cuda")
    for r, p in enumerate(ps):
        re[r, p] = 1.0
    k = np.arange(ln, dtype=np.int64)
    want = np.stack([_twiddle(k * p, ln) for p in ps])
    for got in (d.forward(re), d.forward(re, torch.zeros_like(re))):
        e = row_err(cplx(got), want)
        print(f"DFTERR impulse {dt} L={ln} e={e:.3e} bound={bound(dt, ln):.3e}")
        assert e <= bound(dt, ln)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ln", [3, 1000, 4095])
def test_pure_tones(ln, dt):
    import torch
    d = dft_of(ln)
    k0s = [0, 1, ln - 1]
    n = np.arange(ln, dtype=np.int64)
    z = np.stack([np.conj(_twiddle(k0 * n, ln)) for k0 in k0s])
    re, im = (torch.from_numpy(p.copy()).to(_t(dt)).cuda() for p in (z.real, z.imag))
    got = cplx(d.forward(re, im))
    for r, k0 in enumerate(k0s):
        peak = abs(got[r, k0] - ln)
        rest = np.abs(np.delete(got[r], k0)).max()
        print(f"DFTERR tone {dt} L={ln} k0={k0} peak={peak / ln:.3e} rest={rest / ln:.3e} bound={bound(dt, ln):.3e}")
        assert peak <= bound(dt, ln) * ln and rest <= bound(dt, ln) * ln


@pytest.mark.parametrize("dt", DTS)
def test_zeros_give_exact_zeros(dt):
    import torch
    for ln in (2, 97, 4095):
        d = dft_of(ln)
        zero = torch.zeros((3, ln), dtype=_t(dt), device="cuda")
        for got in (d.forward(zero), d.forward(zero, zero.clone()), d.inverse(zero, zero.clone())):
            assert not got[0].any() and not got[1].any()


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ln", [2, 5, 97, 1000, 2049, 4096])
def test_round_trip(ln, dt):
    d = dft_of(ln)
    re, im, z = gauss(7 * ln, ROWS, ln, dt)
    e = row_err(cplx(d.inverse(*d.forward(re, im))), z)
    print(f"DFTERR roundtrip {dt} L={ln} e={e:.3e} bound={2 * bound(dt, ln):.3e}")
    assert e <= 2 * bound(dt, ln)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ln,rows", [(2, rows_per_wg(32) + 1), (16, rows_per_wg(32) + 1), (17, rows_per_wg(64) + 1),
                                     (32, rows_per_wg(64) + 1), (97, 1), (1000, ROWS), (4095, 1), (4095, 3)])
def test_strides_offsets_and_dead_rows(ln, rows, dt):
    """Row strides L + 3 in and L + 5 out, every base one element into its allocation, batch 1, and one row more than
    a workgroup holds at M = 32 and M = 64 (the last workgroup's other rows are dead); the padding between the rows
    keeps its sentinel."""
    d = dft_of(ln)
    re, im, z = gauss(ln + rows, rows, ln, dt)
    ins = [strided(rows, ln, ln + 3, dt, offset=1) for _ in range(2)]
    outs = [strided(rows, ln, ln + 5, dt, offset=1) for _ in range(2)]
    ins[0][1].copy_(re)
    ins[1][1].copy_(im)
    for inverse, want in ((False, np.fft.fft(z)), (True, np.fft.ifft(z))):
        run = d.inverse if inverse else d.forward
        got = run(ins[0][1], ins[1][1], out=(outs[0][1], outs[1][1]))
        assert got[0].data_ptr() == outs[0][1].data_ptr() and got[1].data_ptr() == outs[1][1].data_ptr()
        assert all(padding_untouched(b, v) for b, v in ins + outs)
        assert row_err(cplx(got), want) <= bound(dt, ln)
        assert same_bits(got, run(re, im))  # the contiguous call
        assert same_bits((ins[0][1], ins[1][1]), (re, im))  # the inputs are read only


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ln", [5, 33, 1000, 4095])
def test_a_row_does_not_depend_on_its_batch(ln, dt):
    d = dft_of(ln)
    re, im, _ = gauss(3 * ln, ROWS, ln, dt)
    full = d.forward(re, im)
    assert same_bits(full, d.forward(re, im))  # two calls
    _, sre = strided(ROWS, ln, ln + 7, dt)
    _, sim = strided(ROWS, ln, ln + 7, dt)
    sre.copy_(re)
    sim.copy_(im)
    assert same_bits(full, d.forward(sre, sim))
    for r in (0, 17, ROWS - 1):
        alone = d.forward(re[r:r + 1].clone(), im[r:r + 1].clone())
        assert same_bits(alone, (full[0][r:r + 1], full[1][r:r + 1])), r


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ln", [3, 97, 1000, 4096])
def test_exact_in_place(ln, dt):
    d = dft_of(ln)
    for inverse in (False, True):
        run = d.inverse if inverse else d.forward
        re, im, _ = gauss(5 * ln, ROWS, ln, dt)
        want = run(re, im)
        _, sre = strided(ROWS, ln, ln + 3, dt)
        _, sim = strided(ROWS, ln, ln + 3, dt)
        sre.copy_(re)
        sim.copy_(im)
        got = run(sre, sim, out=(sre, sim))
        assert same_bits(got, want)
        assert same_bits(run(re, im, out=(re, im)), want)


@pytest.mark.parametrize("dt", DTS)
def test_partial_overlaps_are_refused(dt):
    import torch
    from pragma_dsp_amd import _capi, lib
    ln, rows = 97, 5
    d = dft_of(ln)
    fn = lib.pdsp_dft_c2c_f32 if dt == "f32" else lib.pdsp_dft_c2c_f64
    es = 4 if dt == "f32" else 8
    re = torch.full(((rows + 1) * ln,), 1.0, dtype=_t(dt), device="cuda")
    im = torch.full(((rows + 1) * ln,), 2.0, dtype=_t(dt), device="cuda")
    o1 = torch.full((rows * ln,), SENTINEL, dtype=_t(dt), device="cuda")
    o2 = torch.full((rows * ln,), SENTINEL, dtype=_t(dt), device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off * es)  # noqa: E731

    def refused(re_in, im_in, re_out, im_out, in_stride=ln, out_stride=ln, text=b"output overlaps input"):
        assert fn(d._h, rows, re_in, im_in, in_stride, re_out, im_out, out_stride, 0, None) == _capi.ERR_BAD_ARG
        assert lib.pdsp_last_error().startswith(text), lib.pdsp_last_error()

    refused(p(re), p(im), p(re, ln), p(im, ln))      # both outputs one row down their inputs
    refused(p(re), p(im), p(re, ln), p(o2))          # one of them
    refused(p(re), p(im), p(o1), p(im, 1))           # one element
    refused(p(re), p(im), p(im), p(o2))              # re_out == im_in
    refused(p(re), p(im), p(im), p(re))              # the planes exchanged
    refused(p(re), None, p(re), p(o2))               # a real row has no in-place form
    refused(p(re), p(im), p(re), p(im), ln, ln + 1)  # the same bases at different strides
    refused(p(re), p(im), p(o1), p(o1), text=b"the output planes overlap")   # im_out == re_out
    refused(p(re), p(im), p(o1), p(o1, 1), text=b"the output planes overlap")
    torch.cuda.synchronize()
    assert bool((re == 1.0).all()) and bool((im == 2.0).all())
    assert bool(torch.isnan(o1).all()) and bool(torch.isnan(o2).all())
    # the other checks, ahead of any device work as well
    for args, text in (((0, p(re), p(im), ln, p(o1), p(o2), ln), b"batch must be >= 1, got 0"),
                       ((rows, p(re), p(im), ln - 1, p(o1), p(o2), ln), b"strides must be >= L = 97"),
                       ((rows, p(re), p(im), ln, p(o1), p(o2), ln - 1), b"strides must be >= L = 97"),
                       ((rows, None, p(im), ln, p(o1), p(o2), ln), b"null buffer"),
                       ((rows, p(re), p(im), ln, None, p(o2), ln), b"null buffer"),
                       ((rows, p(re), p(im), ln, p(o1), None, ln), b"null buffer"),
                       ((1 << 31, p(re), p(im), ln, p(o1), p(o2), ln), b"batch too large"),
                       ((1 << 40, p(re), p(im), 1 << 40, p(o1), p(o2), ln), b"batch 1099511627776 x stride overflows")):
        assert fn(d._h, *args, 0, None) == _capi.ERR_BAD_ARG
        assert lib.pdsp_last_error().startswith(text), lib.pdsp_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(o1).all()) and bool(torch.isnan(o2).all())


@pytest.mark.parametrize("dt", DTS)
def test_python_form_on_views_and_a_side_stream(dt):
    import torch
    import pragma_dsp_amd as pd
    ln = 1000
    d = dft_of(ln)
    re, im, z = gauss(11, 2 * ROWS, ln + 24, dt)
    vre, vim = re[::2, 8:8 + ln], im[::2, 8:8 + ln]  # every other row, columns 8 ... of wider rows
    assert not vre.is_contiguous()
    want = np.fft.fft(z[::2, 8:8 + ln])
    got = d.forward(vre, vim)
    assert got[0].shape == (ROWS, ln) and row_err(cplx(got), want) <= bound(dt, ln)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        side = d.forward(vre, vim)
        back = d.inverse(*side)
    s.synchronize()
    assert same_bits(side, got)
    assert row_err(cplx(back), z[::2, 8:8 + ln]) <= 2 * bound(dt, ln)
    with pytest.raises(pd.PdspError):
        d.forward(re, im)  # rows of another length
    with pytest.raises(pd.PdspError):
        d.forward(vre, vim.double() if dt == "f32" else vim.float())
    with pytest.raises(pd.PdspError):
        d.forward(vre.t(), vim.t())
    with pytest.raises(pd.PdspError):
        d.inverse(vre, None)


def test_host_forms_against_numpy():
    import pragma_dsp_amd as pd
    rng = np.random.default_rng(5)
    for ln in (2, 3, 17, 1000, 4095, 4096):
        z = rng.standard_normal((3, ln)) + 1j * rng.standard_normal((3, ln))
        got = pd.dft(z)
        assert got.dtype == np.complex128 and got.shape == z.shape
        ef, ei = row_err(got, np.fft.fft(z)), row_err(pd.idft(z), np.fft.ifft(z))
        er = row_err(pd.dft(z.real), np.fft.fft(z.real))
        print(f"DFTERR host f64 L={ln} fwd={ef:.3e} inv={ei:.3e} real={er:.3e} bound={bound('f64', ln):.3e}")
        assert max(ef, ei, er) <= bound("f64", ln)
        assert row_err(pd.dft(z[0]), np.fft.fft(z[0])) <= bound("f64", ln)  # one row, 1-D
    x = rng.standard_normal(1000)
    back = pd.idft(pd.dft(x))
    assert row_err(back, x.astype(np.complex128)) <= 2 * bound("f64", 1000)
    # the host form is the f64 device form
    import torch
    d = dft_of(1000)
    dev = d.forward(torch.from_numpy(x[None]).cuda())
    assert np.array_equal(cplx(dev)[0], pd.dft(x))

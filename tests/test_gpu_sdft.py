"""The sliding DFT on the MI355X (include/pdsp_hip.h, "sliding DFT"; pdsp_sdft_kernel.h) against long double direct
sums (sdft_ref.direct) and, on every frame of the rectangular bins, one long double prefix sum (sdft_ref.sliding).

The bound is sdft_ref.BOUND: 4 x the worst error of the numpy emulation of the kernel's summation order against the
same direct sums, measured on the CPU before any GPU run -- 8.92 u sqrt(N) max|x| in f32 (u = 2^-24) and 8.84 in f64
(u = 2^-53), the windows' weights summing to 1 in magnitude.  The device measured 2.44 (f32; on the sampled frames its
figures are the emulation's to the digit) and 2.84 (f64) at worst: 0.27 and 0.32 of the bound.

Bit identity (tiles, batch, strides, T, hop, the other bins, b + N, call after call), confinement of NaN / Inf to the
frames that hold them, untouched sentinels, the launch refusals, and the host forms.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import sdft_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH = {"f32": torch.float32, "f64": torch.float64}
FWD_TOL = {"f32": 8e-8, "f64": 2.5e-16}  # test_gpu_stft_pair.py's bound of stft_complex, per log2 N of max|X|


def cplx(re, im):
    re, im = re.cpu().numpy(), im.cpu().numpy()
    z = np.empty(re.shape, dtype=np.complex64 if re.dtype == np.float32 else np.complex128)
    z.real, z.imag = re, im
    return z


def strided(x, dtype, pad=5, fill=float("nan")):
    """[rows, T] numpy -> a 2-D view at row stride T + pad over a buffer whose padding holds `fill`."""
    rows, t = x.shape
    buf = torch.full((rows, t + pad), fill, dtype=TORCH[dtype], device=DEV)
    buf[:, :t] = torch.from_numpy(x).to(TORCH[dtype])
    return buf[:, :t]


class tile_chunks:
    """PDSP_SDFT_TILE_CHUNKS for the calls inside (read at every call)."""

    def __init__(self, v):
        self.v = v

    def __enter__(self):
        self.prev = os.environ.get("PDSP_SDFT_TILE_CHUNKS")
        if self.v:
            os.environ["PDSP_SDFT_TILE_CHUNKS"] = str(self.v)
        else:
            os.environ.pop("PDSP_SDFT_TILE_CHUNKS", None)

    def __exit__(self, *a):
        if self.prev is None:
            os.environ.pop("PDSP_SDFT_TILE_CHUNKS", None)
        else:
            os.environ["PDSP_SDFT_TILE_CHUNKS"] = self.prev


# ---- accuracy -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n,win", [(n, w) for n in R.SIZES for w in R.windows_of(n)])
def test_accuracy(pdsp, n, win, dtype):
    worst = worst_all = 0.0
    bins = R.bins_of(n)
    for t in R.lengths(n):
        x = R.signal(n, t)
        xd = strided(x, dtype)  # batch 3 at in_stride = T + 5
        xmax = np.abs(x).max()
        for h in R.hops(n):
            s = pdsp.SlidingDft(n, bins, hop=h, window=win)
            re, im = s.forward(xd)
            f = R.frames_of(n, h, t)
            assert re.shape == im.shape == (R.ROWS, len(bins), f) and s.frames(t) == f
            got = cplx(re, im)
            fr, dre, dim = R.reference(n, t, h, win)
            worst = max(worst, R.err_units(got[:, :, fr], dre, dim, n, dtype, xmax))
            if win == "rect" and h == 1:
                # every frame, against the prefix-sum reference
                for j in (0, 4):
                    sr, si = R.sliding(x, n, bins[j], h)
                    worst_all = max(worst_all, R.err_units(got[:, j], sr, si, n, dtype, xmax))
    print(f"SDFT device {dtype} N={n} {win}: worst {worst:.3f} (all frames of two bins: {worst_all:.3f}) of the bound "
          f"{R.BOUND[dtype]:.2f} u sqrt(N) max|x|")
    assert worst <= R.BOUND[dtype] and worst_all <= R.BOUND[dtype]


def test_no_drift(pdsp):
    n, t, h, bins = 1024, 1 << 20, 4099, (100.0, 12.5)
    x = np.random.default_rng(11).standard_normal((1, t)).astype(np.float32).astype(np.float64)
    s = pdsp.SlidingDft(n, bins, hop=h)
    got = cplx(*s.forward(torch.from_numpy(x).to(torch.float32).to(DEV)))
    f = R.frames_of(n, h, t)
    assert got.shape == (1, 2, f) and f == 256
    q = f // 4
    first, last = np.arange(q), np.arange(f - q, f)
    errs = []
    for fr in (first, last):
        dre, dim = R.direct(x, n, bins, h, "rect", fr)
        errs.append(R.err_units(got[:, :, fr], dre, dim, n, "f32", np.abs(x).max()))
    print(f"SDFT drift: first quarter {errs[0]:.3f}, last quarter {errs[1]:.3f} of {R.BOUND['f32']:.2f}")
    assert errs[0] <= R.BOUND["f32"] and errs[1] <= R.BOUND["f32"]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n", [64, 1024, 16384])
def test_against_stft_complex(pdsp, n, dtype):
    from pragma_dsp_amd.batch import BatchedFft
    plan = BatchedFft(n, DEV, TORCH[dtype])
    t = 3 * n + 7
    full = torch.from_numpy(R.signal(n, t)[0]).to(TORCH[dtype]).to(DEV)
    bins = [0, 1, 5, n // 4, n // 2 - 1, n // 2]
    xmax = float(full.abs().max())
    for h in (1, n // 4):
        # at hop 1 stft_complex writes N / 2 + 1 bins per sample: starts through the first chunk boundary, or the
        # first two round boundaries of a long chunk, are enough of them
        x = full[:n + min(n, 2100) + 7].contiguous() if h == 1 else full
        for win in R.WINDOWS:
            re, im = plan.stft_complex(x, h, win)           # [frames, N/2 + 1]
            want = cplx(re, im)[:, bins].T                  # [K, frames]
            got = cplx(*pdsp.SlidingDft(n, bins, hop=h, window=win).forward(x))
            assert got.shape == want.shape
            tol = R.BOUND[dtype] * R.U[dtype] * math.sqrt(n) * xmax + FWD_TOL[dtype] * math.log2(n) * np.abs(want).max()
            assert np.abs(got - want).max() <= tol, (n, h, win, np.abs(got - want).max() / tol)


# ---- bit for bit ----------------------------------------------------------------------------------------------------

def same(a, b):
    return all(torch.equal(p.view(torch.int64 if p.dtype == torch.float64 else torch.int32),
                           q.view(torch.int64 if q.dtype == torch.float64 else torch.int32)) for p, q in zip(a, b))


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n,win", [(65, "hann"), (1000, "rect"), (4096, "blackman"), (16384, "rect")])
def test_bits_do_not_depend_on_the_call(pdsp, n, win, dtype):
    t = 5 * n + 7
    x = R.signal(n, t, seed=3)
    xd = torch.from_numpy(x).to(TORCH[dtype]).to(DEV)
    bins = list(R.bins_of(n))
    s = pdsp.SlidingDft(n, bins, hop=1, window=win)
    base = s.forward(xd)
    # forced tiles of 1, 2 and 3 chunks against the default; two calls in a row
    for tc in (1, 2, 3):
        with tile_chunks(tc):
            assert same(s.forward(xd), base), tc
    assert same(s.forward(xd), base)
    # batch 1 against batch 3; contiguous against strided (NaN in the padding between rows)
    one = s.forward(xd[1:2].contiguous())
    assert same(one, (base[0][1:2], base[1][1:2]))
    assert same(s.forward(strided(x, dtype)), base)
    # T against T - 5 on the common frames
    short = s.forward(xd[:, :t - 5].contiguous())
    f = R.frames_of(n, 1, t - 5)
    assert same(short, (base[0][..., :f].contiguous(), base[1][..., :f].contiguous()))
    # hop h against hop 1 at the frames m h
    for h in (7, n - 1, n + 1):
        hopped = pdsp.SlidingDft(n, bins, hop=h, window=win).forward(xd)
        assert same(hopped, (base[0][..., ::h].contiguous(), base[1][..., ::h].contiguous())), h
    # a bin alone against the same bin among seven; b against b + N
    for j in (2, 4):
        alone = pdsp.SlidingDft(n, [bins[j]], hop=1, window=win).forward(xd)
        assert same(alone, (base[0][:, j:j + 1].contiguous(), base[1][:, j:j + 1].contiguous())), j
    moved = pdsp.SlidingDft(n, [12.5 + n, -3.0 - n, 1.0 + 2 * n], hop=1, window=win).forward(xd)
    pick = [4, 5, 1]
    assert same(moved, (base[0][:, pick].contiguous(), base[1][:, pick].contiguous()))


# ---- confinement ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n,win", [(100, "hamming"), (4096, "rect"), (16384, "rect")])
def test_a_bad_sample_reaches_exactly_the_frames_that_hold_it(pdsp, n, win, dtype):
    t, h = 4 * n + 9, 3
    x = R.signal(n, t, seed=5)
    s = pdsp.SlidingDft(n, [1.0, 12.5], hop=h, window=win)
    clean = s.forward(torch.from_numpy(x).to(TORCH[dtype]).to(DEV))
    starts = np.arange(R.frames_of(n, h, t)) * h
    for bad, at in ((float("nan"), 2 * n + 5), (float("inf"), n - 1), (float("-inf"), 3 * n)):
        y = x.copy()
        y[1, at] = bad
        got = s.forward(torch.from_numpy(y).to(TORCH[dtype]).to(DEV))
        holds = (starts <= at) & (at < starts + n)
        assert holds.any() and not holds.all()
        for g, c in zip(got, clean):
            g, c = g.cpu().numpy(), c.cpu().numpy()
            assert np.array_equal(g[[0, 2]], c[[0, 2]])
            assert np.array_equal(g[1][:, ~holds], c[1][:, ~holds]), (bad, at)
        gz = cplx(*got)[1][:, holds]
        assert not np.isfinite(gz.real + gz.imag).any(), (bad, at)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_nothing_is_written_beyond_a_series(pdsp, dtype):
    from pragma_dsp_amd import _capi, _device
    n, t, h, bins = 1000, 3 * 1000 + 7, 7, [0.0, 12.5, 999.0]
    x = torch.from_numpy(R.signal(n, t)).to(TORCH[dtype]).to(DEV)
    s = pdsp.SlidingDft(n, bins, hop=h, window="hann")
    f = s.frames(t)
    stride = f + 3
    sent = -12345.0
    ore, oim = (torch.full((R.ROWS * len(bins) * stride + 3,), sent, dtype=TORCH[dtype], device=DEV) for _ in range(2))
    fn = getattr(_capi.lib, "pdsp_sdft_" + dtype)
    _capi.check(fn(s._h, R.ROWS, _device.ptr(x), t, t, _device.ptr(ore), _device.ptr(oim), stride,
                   _device.stream_ptr(x.device)))
    torch.cuda.synchronize()
    want = s.forward(x)
    for o, w in zip((ore, oim), want):
        assert (o[-3:] == sent).all()
        o = o[:-3].reshape(R.ROWS, len(bins), stride)
        assert (o[..., f:] == sent).all() and torch.equal(o[..., :f], w)


# ---- refusals and host forms ----------------------------------------------------------------------------------------

def test_frames_getter_on_a_handle(pdsp):
    for n, h in ((64, 1), (100, 7), (1000, 1001), (2, 5)):
        s = pdsp.SlidingDft(n, [1.0], hop=h)
        assert [s.frames(t) for t in (n - 1, n, n + h - 1, n + h)] == [0, 1, 1, 2]
        assert (s.length, s.hop, s.components, list(s.bins)) == (n, h, 1, [1.0])
    assert pdsp.SlidingDft(64, 2.5, window="blackman").components == 5


def test_launch_refusals(pdsp):
    from pragma_dsp_amd import _capi
    lib = _capi.lib
    n, t, k = 64, 200, 2
    s = pdsp.SlidingDft(n, [1.0, 2.5], hop=3)
    f = s.frames(t)
    x = torch.zeros(2 * t + 64, dtype=torch.float32, device=DEV)
    o = torch.zeros(2 * 2 * k * f + 64, dtype=torch.float32, device=DEV)
    xp, rp, ip = x.data_ptr(), o.data_ptr(), o.data_ptr() + 4 * 2 * k * f
    vp = C.c_void_p
    arg, ln = _capi.ERR_BAD_ARG, _capi.ERR_INPUT_LENGTH
    big = 1 << 61
    for args, code, text in (
            ((2, vp(xp), t, t, None, vp(ip), f), arg, "null buffer"),
            ((2, None, t, t, vp(rp), vp(ip), f), arg, "null buffer"),
            ((2, vp(xp), t, t, vp(rp), None, f), arg, "null buffer"),
            ((0, vp(xp), t, t, vp(rp), vp(ip), f), arg, "batch must be >= 1, got 0"),
            ((2, vp(xp), t, n - 1, vp(rp), vp(ip), f), ln, "sliding DFT rows of 63 samples are shorter than the window of 64"),
            ((2, vp(xp), t - 1, t, vp(rp), vp(ip), f), arg, f"strides must be >= {t} samples in and >= {f} frames out, got in_stride {t - 1}, out_stride {f}"),
            ((2, vp(xp), t, t, vp(rp), vp(ip), f - 1), arg, f"strides must be >= {t} samples in and >= {f} frames out, got in_stride {t}, out_stride {f - 1}"),
            ((big, vp(xp), big, t, vp(rp), vp(ip), f), arg, f"batch {big} x stride overflows"),
            ((2, vp(xp), t, t, vp(rp), vp(ip), big), arg, "batch 2 x stride overflows"),
            ((2, vp(xp), t, t, vp(xp + 4 * (2 * t - 1)), vp(ip), f), arg, "output overlaps input (the sliding DFT has no in-place form)"),
            ((2, vp(xp), t, t, vp(rp), vp(xp), f), arg, "output overlaps input (the sliding DFT has no in-place form)"),
            ((2, vp(xp), t, t, vp(rp), vp(rp + 4 * (2 * k * f - 1)), f), arg, "the output planes overlap each other"),
            ((2, vp(xp), t, t, vp(rp), vp(rp), f), arg, "the output planes overlap each other")):
        rc = lib.pdsp_sdft_f32(s._h, args[0], args[1], args[2], args[3], args[4], args[5], args[6], None)
        assert rc == code and lib.pdsp_last_error().decode() == text, (rc, lib.pdsp_last_error(), text)
    torch.cuda.synchronize()
    assert not o.any()
    # the Python layer's own checks
    E = pdsp.PdspError
    xs = torch.zeros(2, t, dtype=torch.float32, device=DEV)
    for call in (lambda: s.forward(xs.cpu()), lambda: s.forward(xs.half()), lambda: s.forward(xs, out=xs),
                 lambda: s.forward(xs, out=(torch.zeros(2, k, f + 1, device=DEV), torch.zeros(2, k, f + 1, device=DEV))),
                 lambda: s.forward(xs, out=(torch.zeros(2, k, f, device=DEV).double(), torch.zeros(2, k, f, device=DEV))),
                 lambda: s.forward(xs.t().contiguous().t())):
        with pytest.raises(E) as e:
            call()
        assert e.value.code == arg
    with pytest.raises(E) as e:
        s.forward(xs[:, :n - 1].contiguous())
    assert e.value.code == ln


@pytest.mark.parametrize("n,h,win", [(100, 7, "hamming"), (4096, 1, "rect"), (1000, 1001, "blackman")])
def test_host_forms_are_the_device_forms_bits(pdsp, n, h, win):
    t = 3 * n + 7
    x = R.signal(n, t, seed=9)
    bins = [0.0, 12.5, -3.0]
    dev = cplx(*pdsp.SlidingDft(n, bins, hop=h, window=win).forward(torch.from_numpy(x).to(DEV)))
    host = pdsp.sliding_dft(x, n, bins, hop=h, window=win)
    assert host.dtype == np.complex128 and host.shape == dev.shape and np.array_equal(host, dev)
    assert np.array_equal(pdsp.sliding_dft(x[0], n, bins, hop=h, window=win), dev[0])
    assert np.array_equal(pdsp.sliding_dft(x.reshape(3, 1, t), n, bins[1], hop=h, window=win), dev[:, None, 1:2])
    # goertzel: one frame of the whole row
    g = pdsp.goertzel(x[:, :n], bins)
    one = cplx(*pdsp.SlidingDft(n, bins).forward(torch.from_numpy(x[:, :n].copy()).to(DEV)))
    assert g.shape == (3, 3) and np.array_equal(g, one[..., 0])
    dre, dim = R.direct(x[:, :n], n, bins)
    assert R.err_units(g[..., None], dre, dim, n, "f64", np.abs(x).max()) <= R.BOUND["f64"]

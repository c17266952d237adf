"""The complex short-time transform and its overlap-add inverse on the device (BatchedFft.stft_complex / .istft,
pdsp_stft_complex_* / pdsp_istft_*), f32 and f64, against f64 numpy restatements of the contract in
include/pdsp_hip.h computed from the very same inputs:

  forward   X_b = numpy.fft.rfft(w * frame_b), every N = 64 ... 16384, hops 1, N/4, N/4 + 1, N/2, N, N + 3, every
            window type and a table window, zero-padded rows, and torch.stft(center=False) on a few shapes;
  inverse   y_b = irfft(X_b, N) (imaginary parts of bins 0 and N/2 ignored), out = sum w y_b / sum w^2 in ascending
            b, exact 0 where the denominator is <= 1e-11;
  round trip, bit-identical repeats and chunk sizes, guard bands, dead rows, refused aliasing, argument errors.

Error metrics (stated as FIR's were, scaled with log2 N): forward max|X - X_ref| / max|X_ref| per call; inverse
max |out - ref| sqrt(den) / (max|y| sqrt(K)) over samples with den >= 1e-3 max den, K = ceil(N / hop) frames per
sample -- the numerator's error scale, so that the division by a small den is not counted as the kernel's error."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1 << k for k in range(6, 15)]
WINDOWS = ["rect", "hann", "hamming", "blackman"]
DTYPES = [torch.float32, torch.float64]
# bounds per log2 N, about 3x the worst error measured on an MI355X over these tests:
# forward 2.7e-8 / 8.1e-17, inverse 2.3e-8 / 7.4e-17, round trip 3.5e-8 / 5.1e-17 (f32 / f64)
FWD_TOL = {torch.float32: 8e-8, torch.float64: 2.5e-16}
INV_TOL = {torch.float32: 7e-8, torch.float64: 2.2e-16}
RT_TOL = {torch.float32: 1e-7, torch.float64: 1.6e-16}
THR = 1e-11


@pytest.fixture(scope="module")
def plans():
    from pragma_dsp_amd.batch import BatchedFft
    cache = {}

    def get(n, dtype):
        key = (n, dtype)
        if key not in cache:
            cache[key] = BatchedFft(n, "cuda:0", dtype)
        return cache[key]

    yield get
    for p in cache.values():
        p.close()


def win64(plan, window):
    """The window the kernel multiplies by, in f64: the plan's table rounded to its dtype, or the caller's tensor."""
    if isinstance(window, str):
        if window == "rect":
            return np.ones(plan.size)
        return plan.window(window).tensor().cpu().numpy().astype(np.float64)
    return window.cpu().numpy().astype(np.float64)


def ref_stft(x64, n, hop, w):
    frames = 1 + (x64.size - n) // hop
    idx = np.arange(frames)[:, None] * hop + np.arange(n)[None, :]
    return np.fft.rfft(x64[idx] * w[None, :], axis=1)


def ref_istft(spec, n, hop, w):
    """f64 restatement of the inverse: (out, den)."""
    z = np.array(spec, dtype=np.complex128)
    z[:, 0] = z[:, 0].real
    z[:, -1] = z[:, -1].real
    y = np.fft.irfft(z, n, axis=1)
    frames = z.shape[0]
    total = (frames - 1) * hop + n
    num, den = np.zeros(total), np.zeros(total)
    for b in range(frames):  # ascending b
        num[b * hop:b * hop + n] += w * y[b]
        den[b * hop:b * hop + n] += w * w
    out = np.where(den > THR, num / np.where(den > THR, den, 1.0), 0.0)
    return out, den, np.abs(y).max()


def hops_for(n):
    return [1, n // 4, n // 4 + 1, n // 2, n, n + 3]


def to_np(t):
    return t.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n", SIZES)
def test_forward_matches_rfft_of_windowed_frames(plans, n, dtype):
    plan = plans(n, dtype)
    rng = np.random.default_rng(n + (7 if dtype == torch.float64 else 0))
    table = torch.from_numpy(rng.uniform(0.1, 1.0, n)).to(dtype).cuda()
    lg = math.log2(n)
    for hop in hops_for(n):
        frames = 5 if hop == 1 else 9
        length = n + (frames - 1) * hop + (hop - 1 if hop > 1 else 0)  # a tail shorter than a hop is ignored
        x = torch.from_numpy(rng.standard_normal(length)).to(dtype).cuda()
        x64 = to_np(x)
        for window in WINDOWS + [table]:
            re, im = plan.stft_complex(x, hop, window)
            assert re.shape == im.shape == (frames, n // 2 + 1)
            want = ref_stft(x64, n, hop, win64(plan, window))
            got = to_np(re) + 1j * to_np(im)
            err = np.abs(got - want).max() / np.abs(want).max()
            assert err <= FWD_TOL[dtype] * lg, (n, hop, window if isinstance(window, str) else "table", err)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n", [64, 1024, 16384])
def test_forward_zero_padded_rows(plans, n, dtype):
    """frame_len < N on contiguous rows (frame_stride = frame_len): a row-wise one-sided transform of padded rows."""
    from pragma_dsp_amd import _capi
    plan = plans(n, dtype)
    sfx = "f32" if dtype == torch.float32 else "f64"
    rng = np.random.default_rng(5)
    for flen in (1, n // 2 - 3, n - 1):
        rows = 37
        x = torch.from_numpy(rng.standard_normal(rows * flen)).to(dtype).cuda()
        win = plan.window("hann")
        re = torch.empty((rows, n // 2 + 1), dtype=dtype, device="cuda:0")
        im = torch.empty_like(re)
        _capi.check(getattr(_capi.lib, "pdsp_stft_complex_" + sfx)(plan._h, rows, C.c_void_p(x.data_ptr()), flen, flen,
                                                                   C.c_void_p(win.data_ptr()), C.c_void_p(re.data_ptr()),
                                                                   C.c_void_p(im.data_ptr()), None))
        padded = np.zeros((rows, n))
        padded[:, :flen] = to_np(x).reshape(rows, flen)
        want = np.fft.rfft(padded * win64(plan, "hann")[None, :], axis=1)
        got = to_np(re) + 1j * to_np(im)
        assert np.abs(got - want).max() <= FWD_TOL[dtype] * math.log2(n) * max(np.abs(want).max(), 1e-30), (n, flen)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_forward_agrees_with_torch_stft(plans, dtype):
    rng = np.random.default_rng(11)
    for n, hop, window in ((256, 64, "hann"), (1024, 1024, "rect"), (4096, 1000, "hamming"), (16384, 4096, "blackman")):
        plan = plans(n, dtype)
        x = torch.from_numpy(rng.standard_normal(n + 6 * hop + 17)).to(dtype).cuda()
        re, im = plan.stft_complex(x, hop, window)
        w = torch.from_numpy(win64(plan, window)).to(dtype).cuda()
        t = torch.stft(x, n_fft=n, hop_length=hop, win_length=n, window=w, center=False, onesided=True,
                       return_complex=True).transpose(0, 1)
        got = torch.complex(re, im)
        err = ((got - t).abs().max() / t.abs().max()).item()
        assert err <= 2 * FWD_TOL[dtype] * math.log2(n), (n, hop, window, err)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n", [64, 256, 1024, 4096, 16384])
def test_inverse_matches_the_definition(plans, n, dtype):
    plan = plans(n, dtype)
    rng = np.random.default_rng(3 * n + 1)
    lg = math.log2(n)
    table = torch.from_numpy(rng.uniform(0.1, 1.0, n)).to(dtype).cuda()
    for hop in hops_for(n):
        frames = 4 if hop == 1 else 7
        bins = n // 2 + 1
        re = torch.from_numpy(rng.standard_normal((frames, bins))).to(dtype).cuda()
        im = torch.from_numpy(rng.standard_normal((frames, bins))).to(dtype).cuda()
        for window in WINDOWS + [table]:
            w = win64(plan, window)
            out = plan.istft(re, im, hop, window)
            want, den, ymax = ref_istft(to_np(re) + 1j * to_np(im), n, hop, w)
            got = to_np(out)
            assert got.shape == want.shape
            clear = np.abs(den - THR) > 1e-4 * THR
            zero = (den <= THR) & clear
            assert np.all(got[zero] == 0.0), (n, hop, "the 1e-11 threshold and the gaps are exact zeros")
            good = den >= 1e-3 * den.max()
            k = math.ceil(n / hop)
            err = (np.abs(got - want)[good] * np.sqrt(den[good])).max() / (ymax * math.sqrt(k))
            assert err <= INV_TOL[dtype] * lg, (n, hop, window if isinstance(window, str) else "table", err)
            if hop > n:  # the gaps behind every frame but the last are zero
                for b in range(frames - 1):
                    assert np.all(got[b * hop + n:(b + 1) * hop] == 0.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_inverse_sums_in_ascending_frame_order(plans, dtype):
    """The sum order is part of the contract.  The device's own frames y_b come back exactly from the rect inverse at
    hop = N (den = 1: out = y_b / 1); with rect at hop < N, den is the count of frames and out[t] must equal
    (0 + y_b0 + y_b1 + ...) / count summed in ascending b in the output's precision, bit for bit.  Frames of very
    different scales make any other order visible."""
    n, hop, frames = 256, 48, 11
    plan = plans(n, dtype)
    rng = np.random.default_rng(29)
    scale = (10.0 ** rng.uniform(-6, 6, frames))[:, None]
    re = torch.from_numpy(rng.standard_normal((frames, n // 2 + 1)) * scale).to(dtype).cuda()
    im = torch.from_numpy(rng.standard_normal((frames, n // 2 + 1)) * scale).to(dtype).cuda()
    y = plan.istft(re, im, n, "rect").cpu().numpy().reshape(frames, n)
    got = plan.istft(re, im, hop, "rect").cpu().numpy()
    npdt = y.dtype.type
    want = np.zeros(got.size, dtype=y.dtype)
    for t in range(got.size):
        num, den = npdt(0), npdt(0)
        for b in range(frames):
            if b * hop <= t < b * hop + n:
                num = npdt(num + y[b, t - b * hop])
                den = npdt(den + npdt(1))
        want[t] = npdt(num / den)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("n", [64, 1024, 16384])
def test_round_trip(plans, n, dtype):
    plan = plans(n, dtype)
    rng = np.random.default_rng(n)
    for hop in (n // 4, n // 2, n, n // 4 + 1):
        for window in WINDOWS:
            x = torch.from_numpy(rng.standard_normal(n + 9 * hop)).to(dtype).cuda()
            re, im = plan.stft_complex(x, hop, window)
            out = to_np(plan.istft(re, im, hop, window))
            w = win64(plan, window)
            _, den, _ = ref_istft(np.zeros((re.shape[0], n // 2 + 1)), n, hop, w)
            x64 = to_np(x)[:out.size]
            ok = den > THR * (1 + 1e-4)
            k = math.ceil(n / hop)
            err = (np.abs(out - x64)[ok] * np.sqrt(den[ok])).max() / (np.abs(x64).max() * math.sqrt(k))
            assert err <= RT_TOL[dtype] * math.log2(n), (n, hop, window, err)
            assert np.all(out[den <= THR * (1 - 1e-4)] == 0.0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_rect_hop_n_is_rowwise_irfft(plans, dtype):
    n, frames = 1024, 33
    plan = plans(n, dtype)
    rng = np.random.default_rng(2)
    re = torch.from_numpy(rng.standard_normal((frames, n // 2 + 1))).to(dtype).cuda()
    im = torch.from_numpy(rng.standard_normal((frames, n // 2 + 1))).to(dtype).cuda()
    out = plan.istft(re, im, n, "rect")
    z = to_np(re) + 1j * to_np(im)
    want = np.fft.irfft(z, n, axis=1).reshape(-1)
    assert np.abs(to_np(out) - want).max() <= INV_TOL[dtype] * 10 * np.abs(want).max()
    # the same frames with gaps of 3 between them: the frames bit for bit, the gaps exactly 0
    gapped = plan.istft(re, im, n + 3, "rect").cpu()
    rows = torch.stack([gapped[b * (n + 3):b * (n + 3) + n] for b in range(frames)]).reshape(-1)
    assert torch.equal(rows, out.cpu())
    assert all(torch.all(gapped[b * (n + 3) + n:(b + 1) * (n + 3)] == 0) for b in range(frames - 1))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_bit_identical_repeats_and_chunk_sizes(plans, dtype):
    from pragma_dsp_amd import _capi
    rng = np.random.default_rng(17)
    for n, hop, frames in ((64, 16, 301), (1024, 100, 97), (4096, 1024, 40), (16384, 1, 12)):
        plan = plans(n, dtype)
        re = torch.from_numpy(rng.standard_normal((frames, n // 2 + 1))).to(dtype).cuda()
        im = torch.from_numpy(rng.standard_normal((frames, n // 2 + 1))).to(dtype).cuda()
        first = plan.istft(re, im, hop, "hann")
        for _ in range(2):
            assert torch.equal(plan.istft(re, im, hop, "hann"), first), (n, hop)
        prev = _capi.lib.pdsp_set_istft_chunk_frames(1)
        try:
            for s in (1, 7, 0):
                _capi.lib.pdsp_set_istft_chunk_frames(s)
                assert torch.equal(plan.istft(re, im, hop, "hann"), first), (n, hop, s)
        finally:
            _capi.lib.pdsp_set_istft_chunk_frames(prev)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_guard_bands_and_dead_rows(plans, dtype):
    """Outputs written through raw pointers into the middle of NaN-filled buffers: nothing outside them changes.
    Frame counts that leave the last workgroup mostly dead (N = 64: 128 frames per workgroup)."""
    from pragma_dsp_amd import _capi
    sfx = "f32" if dtype == torch.float32 else "f64"
    guard = 4096
    rng = np.random.default_rng(23)
    for n, frames, hop in ((64, 129, 16), (64, 129, 64), (64, 130, 67), (256, 33, 256), (2048, 3, 512), (16384, 2, 8192)):
        plan = plans(n, dtype)
        bins = n // 2 + 1
        x = torch.from_numpy(rng.standard_normal(n + (frames - 1) * hop)).to(dtype).cuda()
        buf = torch.full((2 * frames * bins + 3 * guard,), float("nan"), dtype=dtype, device="cuda:0")
        re, im = buf[guard:guard + frames * bins], buf[2 * guard + frames * bins:2 * guard + 2 * frames * bins]
        win = plan.window("hann")
        _capi.check(getattr(_capi.lib, "pdsp_stft_complex_" + sfx)(plan._h, frames, C.c_void_p(x.data_ptr()), n, hop,
                                                                   C.c_void_p(win.data_ptr()), C.c_void_p(re.data_ptr()),
                                                                   C.c_void_p(im.data_ptr()), None))
        torch.cuda.synchronize()
        assert torch.isnan(buf[:guard]).all() and torch.isnan(buf[guard + frames * bins:2 * guard + frames * bins]).all()
        assert torch.isnan(buf[2 * guard + 2 * frames * bins:]).all()
        assert not torch.isnan(re).any() and not torch.isnan(im).any()
        want = ref_stft(to_np(x), n, hop, win64(plan, "hann"))
        got = to_np(re).reshape(frames, bins) + 1j * to_np(im).reshape(frames, bins)
        assert np.abs(got - want).max() <= FWD_TOL[dtype] * math.log2(n) * np.abs(want).max()
        total = (frames - 1) * hop + n
        obuf = torch.full((total + 2 * guard,), float("nan"), dtype=dtype, device="cuda:0")
        rc, ic = re.reshape(frames, bins).contiguous(), im.reshape(frames, bins).contiguous()
        _capi.check(getattr(_capi.lib, "pdsp_istft_" + sfx)(plan._h, frames, C.c_void_p(rc.data_ptr()), C.c_void_p(ic.data_ptr()),
                                                            hop, C.c_void_p(win.data_ptr()),
                                                            C.c_void_p(obuf[guard:].data_ptr()), None))
        torch.cuda.synchronize()
        assert torch.isnan(obuf[:guard]).all() and torch.isnan(obuf[guard + total:]).all()
        assert not torch.isnan(obuf[guard:guard + total]).any()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_output_overlapping_an_input_is_refused(plans, dtype):
    from pragma_dsp_amd import _capi
    sfx = "f32" if dtype == torch.float32 else "f64"
    n, frames, hop = 256, 8, 64
    plan = plans(n, dtype)
    bins = n // 2 + 1
    buf = torch.zeros(4 * frames * bins + 4 * n, dtype=dtype, device="cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    sig = buf[:n + (frames - 1) * hop]
    fwd = getattr(_capi.lib, "pdsp_stft_complex_" + sfx)
    inv = getattr(_capi.lib, "pdsp_istft_" + sfx)
    # re_out starting inside the signal's last sample; im_out meeting re_out; both past it but on the window
    end = sig.numel()
    assert fwd(plan._h, frames, p(sig), n, hop, None, p(buf[end - 1:]), p(buf[end + 2 * frames * bins:]), None) == _capi.ERR_BAD_ARG
    assert _capi.lib.pdsp_last_error() == b"output overlaps input"
    assert fwd(plan._h, frames, p(sig), n, hop, None, p(buf[end:]), p(buf[end + frames * bins - 1:]), None) == _capi.ERR_BAD_ARG
    win = buf[end + 3 * frames * bins:end + 3 * frames * bins + n]
    assert fwd(plan._h, frames, p(sig), n, hop, p(win), p(buf[end:]), p(win[n - 1:]), None) == _capi.ERR_BAD_ARG
    re, im = buf[:frames * bins], buf[frames * bins:2 * frames * bins]
    assert inv(plan._h, frames, p(re), p(im), hop, None, p(buf[2 * frames * bins - 1:]), None) == _capi.ERR_BAD_ARG
    assert inv(plan._h, frames, p(re), p(im), hop, None, p(re), None) == _capi.ERR_BAD_ARG
    assert _capi.lib.pdsp_last_error() == b"output overlaps input"
    # one element further on: accepted
    assert inv(plan._h, frames, p(re), p(im), hop, None, p(buf[2 * frames * bins:]), None) == _capi.OK
    torch.cuda.synchronize()


def test_device_entries_check_size_range_and_counts(plans):
    from pragma_dsp_amd import _capi
    from pragma_dsp_amd.batch import BatchedFft
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for n in (32, 32768):
        plan = BatchedFft(n, "cuda:0")
        x = torch.zeros(2 * n, device="cuda:0")
        assert _capi.lib.pdsp_stft_complex_f32(plan._h, 1, p(x), n, n, None, p(x), p(x), None) == _capi.ERR_UNSUPPORTED_SIZE
        assert _capi.lib.pdsp_last_error() == f"STFT needs a plan of 64 <= N <= 16384, got {n}".encode()
        assert _capi.lib.pdsp_istft_f32(plan._h, 1, p(x), p(x), 4, None, p(x), None) == _capi.ERR_UNSUPPORTED_SIZE
        plan.close()
    plan = plans(256, torch.float32)
    x = torch.zeros(4096, device="cuda:0")
    y = torch.zeros(4096, device="cuda:0")
    lib = _capi.lib
    assert lib.pdsp_stft_complex_f32(plan._h, 0, p(x), 256, 64, None, p(y), p(y[2048:]), None) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"frames must be >= 1, got 0"
    assert lib.pdsp_stft_complex_f32(plan._h, 2, p(x), 256, 0, None, p(y), p(y[2048:]), None) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"frame_stride (hop) must be >= 1, got 0"
    assert lib.pdsp_stft_complex_f32(plan._h, 1 << 31, p(x), 256, 64, None, p(y), p(y[2048:]), None) == _capi.ERR_BAD_ARG
    assert lib.pdsp_stft_complex_f32(plan._h, (1 << 30), p(x), 256, 1 << 40, None, p(y), p(y[2048:]), None) == _capi.ERR_BAD_ARG
    assert b"overflows" in lib.pdsp_last_error()
    assert lib.pdsp_istft_f32(plan._h, 0, p(x), p(x), 64, None, p(y), None) == _capi.ERR_BAD_ARG
    assert lib.pdsp_istft_f32(plan._h, 2, p(x), p(x), 0, None, p(y), None) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"hop must be >= 1, got 0"
    assert lib.pdsp_istft_f32(plan._h, 1 << 31, p(x), p(x), 1, None, p(y), None) == _capi.ERR_BAD_ARG
    assert lib.pdsp_istft_f32(plan._h, 1 << 30, p(x), p(x), 1 << 40, None, p(y), None) == _capi.ERR_BAD_ARG
    assert b"overflows" in lib.pdsp_last_error()
    assert lib.pdsp_istft_f32(plan._h, 2, None, p(x), 64, None, p(y), None) == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == b"null buffer"


def test_python_argument_errors(plans):
    from pragma_dsp_amd import _capi
    from pragma_dsp_amd._capi import PdspError
    n = 256
    plan = plans(n, torch.float32)
    other = plans(n, torch.float64)
    sig = torch.zeros(4 * n, device="cuda:0")
    re, im = plan.stft_complex(sig, 64)
    frames = re.shape[0]
    total = (frames - 1) * 64 + n
    bad = [
        (lambda: plan.stft_complex(sig.double(), 64), _capi.ERR_BAD_ARG),
        (lambda: plan.stft_complex(sig.cpu(), 64), _capi.ERR_BAD_ARG),
        (lambda: plan.stft_complex(sig.reshape(4, n), 64), _capi.ERR_BAD_ARG),
        (lambda: plan.stft_complex(sig[::2], 64), _capi.ERR_BAD_ARG),
        (lambda: plan.stft_complex(sig, 0), _capi.ERR_BAD_ARG),
        (lambda: plan.stft_complex(sig[:n - 1], 64), _capi.ERR_INPUT_LENGTH),
        (lambda: plan.stft_complex(sig, 64, "kaiser"), _capi.ERR_WINDOW_TYPE),
        (lambda: plan.stft_complex(sig, 64, torch.ones(n - 1, device="cuda:0")), _capi.ERR_WINDOW_LENGTH),
        (lambda: plan.stft_complex(sig, 64, torch.ones(n, device="cuda:0", dtype=torch.float64)), _capi.ERR_BAD_ARG),
        (lambda: plan.stft_complex(sig, 64, other.window("hann")), _capi.ERR_BAD_ARG),
        (lambda: plan.stft_complex(sig, 64, [1.0] * n), _capi.ERR_BAD_ARG),
        (lambda: plan.istft(re, im[:, :-1].contiguous(), 64), _capi.ERR_INPUT_LENGTH),
        (lambda: plan.istft(re, im[:-1], 64), _capi.ERR_BAD_ARG),
        (lambda: plan.istft(re.reshape(-1), im.reshape(-1), 64), _capi.ERR_BAD_ARG),
        (lambda: plan.istft(re.double(), im.double(), 64), _capi.ERR_BAD_ARG),
        (lambda: plan.istft(re.cpu(), im.cpu(), 64), _capi.ERR_BAD_ARG),
        (lambda: plan.istft(re.t().contiguous().t(), im, 64), _capi.ERR_BAD_ARG),
        (lambda: plan.istft(re[:0], im[:0], 64), _capi.ERR_BAD_ARG),
        (lambda: plan.istft(re, im, 0), _capi.ERR_BAD_ARG),
        (lambda: plan.istft(re, im, 64, out=torch.empty(total + 1, device="cuda:0")), _capi.ERR_INPUT_LENGTH),
        (lambda: plan.istft(re, im, 64, out=torch.empty(total, device="cuda:0", dtype=torch.float64)), _capi.ERR_BAD_ARG),
        (lambda: plan.istft(re, im, 64, out=torch.empty((1, total), device="cuda:0")), _capi.ERR_BAD_ARG),
        (lambda: plan.istft(re, im, 64, "welch"), _capi.ERR_WINDOW_TYPE),
    ]
    for i, (call, code) in enumerate(bad):
        with pytest.raises(PdspError) as e:
            call()
        assert e.value.code == code, (i, str(e.value))
    out = torch.full((total,), float("nan"), device="cuda:0")
    assert plan.istft(re, im, 64, out=out) is out and not torch.isnan(out).any()

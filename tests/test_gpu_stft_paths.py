"""The complex short-time pair instantiation by instantiation and at full overlap: stft_complex_kernel,
istft_frame_kernel and istft_ola_kernel (pdsp_stft_kernel.h) and the chunked host loop (pdsp_kernels_stft.hip).
test_gpu_stft_pair.py states the contract, the references (numpy.fft.rfft / irfft in f64 on the dtype-rounded inputs),
the two metrics and their bounds; this file imports them unchanged and runs them where that file does not reach:

  a  every istft_frame_kernel<T, LOG2M, HAS_WIN, DIRECT> (9 sizes x 2 types x 2 window forms x 2 DIRECT forms) against
     ref_istft, gaps longer than a row's thread count exactly zero, gapped frames = hop-N frames bit for bit;
  b  every stft_complex_kernel<T, LOG2M, HAS_WIN> with frame_len < N (zero padded) and frame_len > N (truncated);
  c  the tables of a and b (and of the pair file's forward test) reach all 112 instantiations;
  d  the overlap-add at depths of 22 ... 128 frames per sample, bit-identical for chunk sizes 1, K, K + 1, 2K + 3;
  e  the default chunk size S crossed without the development switch;
  f  one and two frames, dead rows of the last workgroup, values and margins;
  g  every buffer one element past a 16-byte boundary;
  h  non-finite imaginary parts of bins 0 and N/2 are ignored;
  i  a non-finite sample or bin stays in the frames / samples it belongs to;
  j  torch.istft(center=False, onesided=True) on the CPU;
  k  the round trip at every size;
  l  the host forms pragma_dsp_amd.stft / istft against the references and BatchedFft's bits.

The mapping from a call to its instantiation (test c) restates istft_dev / stft_complex_dev: HAS_WIN = a window pointer
was passed ("rect" passes none), DIRECT = hop >= N, LOG2M = log2 N - 1; istft_ola_kernel<T, HAS_WIN> runs when hop < N.
Every test prints one STFTERR line (what it measured, its share of the bound) before it asserts."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import test_gpu_stft_pair as pair
from test_gpu_dct import rows_per_wg
from test_gpu_stft_pair import FWD_TOL, INV_TOL, RT_TOL, THR, plans, ref_istft, ref_stft, to_np, win64  # noqa: F401

pytestmark = pytest.mark.gpu

SIZES = [1 << k for k in range(6, 15)]
DTYPES = [torch.float32, torch.float64]
DT_IDS = ["f32", "f64"]
SFX = {torch.float32: "f32", torch.float64: "f64"}
NAN = float("nan")
GUARD = 4096

# the parameter tables of cases a and b; test c computes the instantiations they reach from these
A_WINDOWS = ["rect", "hann", "table"]
B_WINDOWS = ["rect", "table"]


def a_hops(n):
    return [n // 4 + 1, n, 2 * n + 5]


def b_lens(n):
    return [1, 2, n // 2, n // 2 + 1, n - 1]


def inverse_insts(n, dtype, window, hop):
    """istft_dev: `window ? ...`, `hop >= n`, `log2n - 1`; the gather kernel only when frames overlap."""
    has_win, direct, log2m = window != "rect", hop >= n, n.bit_length() - 2
    reached = {("istft_frame_kernel", dtype, log2m, has_win, direct)}
    if not direct:
        reached.add(("istft_ola_kernel", dtype, None, has_win, None))
    return reached


def forward_inst(n, dtype, window):
    """stft_complex_dev: `window ? ...`, `log2n - 1`."""
    return ("stft_complex_kernel", dtype, n.bit_length() - 2, window != "rect", None)


class Tally:
    """The worst figure of one test against its bound, and its exact checks; done() prints the STFTERR line, then
    asserts."""

    def __init__(self, case, kind, dtype, n):
        self.head = f"STFTERR case={case} kind={kind} dtype={SFX[dtype]} n={n}"
        self.lg = math.log2(n)
        self.err, self.share, self.where, self.fails, self.exacts = 0.0, 0.0, None, [], 0

    def add(self, err, tol, where):
        bound = tol * self.lg
        if not err <= bound:  # a NaN fails
            self.fails.append((where, float(err), bound))
        if not err / bound <= self.share:
            self.err, self.share, self.where = float(err), float(err / bound), where

    def exact(self, ok, where):
        self.exacts += 1
        if not ok:
            self.fails.append((where, "not exact"))

    def done(self):
        print(f"{self.head} err={self.err:.3e} per_log2n={self.err / self.lg:.3e} share={self.share:.3f} at={self.where} "
              f"exact_checks={self.exacts} failed={len(self.fails)}")
        assert not self.fails, self.fails[:8]


def inv_err(got, want, den, ymax, n, hop):
    """The pair file's inverse metric: max|out - ref| sqrt(den) / (max|y| sqrt(K)) over den >= 1e-3 max den."""
    good = den >= 1e-3 * den.max()
    return (np.abs(got - want)[good] * np.sqrt(den[good])).max() / (ymax * math.sqrt(math.ceil(n / hop)))


def zeros_where_den_small(got, den):
    clear = np.abs(den - THR) > 1e-4 * THR
    return bool(np.all(got[(den <= THR) & clear] == 0.0))


def gauss(rng, shape, dtype):
    return torch.from_numpy(rng.standard_normal(shape)).to(dtype).cuda()


def table_window(rng, n, dtype):
    return torch.from_numpy(rng.uniform(0.1, 1.0, n)).to(dtype).cuda()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def win_arg(plan, window):
    """The pointer operand of the C ABI for a window of the Python layer: none for "rect", the plan's table for a name."""
    if isinstance(window, str):
        return None if window == "rect" else plan.window(window)
    return window


def raw_stft(plan, dtype, batch, x, frame_len, stride, win, re, im):
    from pragma_dsp_amd import _capi
    _capi.check(getattr(_capi.lib, "pdsp_stft_complex_" + SFX[dtype])(plan._h, batch, ptr(x), frame_len, stride, ptr(win),
                                                                    ptr(re), ptr(im), None))


def raw_istft(plan, dtype, frames, re, im, hop, win, out):
    from pragma_dsp_amd import _capi
    _capi.check(getattr(_capi.lib, "pdsp_istft_" + SFX[dtype])(plan._h, frames, ptr(re), ptr(im), hop, ptr(win), ptr(out),
                                                             None))


def istft_filled(plan, re, im, hop, window):
    """plan.istft into a NaN-filled output: a sample that no thread writes shows, whatever the allocator hands out."""
    total = (re.shape[0] - 1) * hop + plan.size
    return plan.istft(re, im, hop, window, out=torch.full((total,), NAN, dtype=re.dtype, device=re.device))


def set_chunk(frames):
    from pragma_dsp_amd import _capi
    return _capi.lib.pdsp_set_istft_chunk_frames(frames)


# ---- a ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", SIZES)
def test_a_every_inverse_instantiation(plans, n, dtype):
    plan = plans(n, dtype)
    rng = np.random.default_rng(5 * n + SFX[dtype].count("6"))
    frames, bins = 7, n // 2 + 1
    table = table_window(rng, n, dtype)
    re, im = gauss(rng, (frames, bins), dtype), gauss(rng, (frames, bins), dtype)
    spec = to_np(re) + 1j * to_np(im)
    t = Tally("a", "inverse", dtype, n)
    for wname in A_WINDOWS:
        window = table if wname == "table" else wname
        w = win64(plan, window)
        outs = {}
        for hop in a_hops(n):
            outs[hop] = istft_filled(plan, re, im, hop, window).cpu()
            got = outs[hop].numpy().astype(np.float64)
            want, den, ymax = ref_istft(spec, n, hop, w)
            assert got.shape == want.shape
            t.exact(zeros_where_den_small(got, den), (wname, hop, "zeros where den <= 1e-11"))
            t.add(inv_err(got, want, den, ymax, n, hop), INV_TOL[dtype], (wname, hop))
        hop = 2 * n + 5  # a gap of N + 5 > TP samples behind every frame but the last
        gapped = outs[hop]
        t.exact(all(bool(torch.all(gapped[b * hop + n:(b + 1) * hop] == 0)) for b in range(frames - 1)), (wname, "gaps"))
        rows = torch.stack([gapped[b * hop:b * hop + n] for b in range(frames)]).reshape(-1)
        t.exact(torch.equal(rows, outs[n]), (wname, "gapped frames = hop-N frames"))
    t.done()


# ---- b ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", SIZES)
def test_b_forward_short_and_long_frames(plans, n, dtype):
    plan = plans(n, dtype)
    rng = np.random.default_rng(7 * n + SFX[dtype].count("6"))
    rows, bins = 37, n // 2 + 1
    table = table_window(rng, n, dtype)
    t = Tally("b", "forward", dtype, n)

    def run(x, flen, stride, win):
        re = torch.full((rows, bins), NAN, dtype=dtype, device="cuda:0")
        im = torch.full((rows, bins), NAN, dtype=dtype, device="cuda:0")
        raw_stft(plan, dtype, rows, x, flen, stride, win, re, im)
        return re.cpu(), im.cpu()

    for wname in B_WINDOWS:
        win = table if wname == "table" else None
        w = win64(plan, table if wname == "table" else "rect")
        for flen in b_lens(n):  # contiguous rows of frame_len samples, zero padded to N
            x = gauss(rng, rows * flen, dtype)
            re, im = run(x, flen, flen, win)
            padded = np.zeros((rows, n))
            padded[:, :flen] = to_np(x).reshape(rows, flen)
            want = np.fft.rfft(padded * w[None, :], axis=1)
            got = to_np(re) + 1j * to_np(im)
            t.add(np.abs(got - want).max() / np.abs(want).max(), FWD_TOL[dtype], (wname, flen))
        stride = n + 5  # frame_len > N: the first N samples of each row
        x = gauss(rng, rows * stride, dtype)
        long_re, long_im = run(x, n + 5, stride, win)
        re, im = run(x, n, stride, win)
        t.exact(torch.equal(long_re, re) and torch.equal(long_im, im), (wname, "frame_len N + 5 = frame_len N"))
        want = np.fft.rfft(to_np(x).reshape(rows, stride)[:, :n] * w[None, :], axis=1)
        got = to_np(long_re) + 1j * to_np(long_im)
        t.add(np.abs(got - want).max() / np.abs(want).max(), FWD_TOL[dtype], (wname, n + 5))
    t.done()


# ---- c ------------------------------------------------------------------------------------------------------------

def test_c_tables_reach_every_instantiation():
    """The instantiations that the tables of a, b and test_forward_matches_rfft_of_windowed_frames reach, without
    running them: the full product, 72 istft_frame_kernel + 36 stft_complex_kernel + 4 istft_ola_kernel."""
    seen = set()
    for n in SIZES:
        for dtype in DTYPES:
            for window in A_WINDOWS:
                for hop in a_hops(n):
                    seen |= inverse_insts(n, dtype, window, hop)
            for window in B_WINDOWS:
                seen.add(forward_inst(n, dtype, window))
    marks = {m.args[0]: m.args[1] for m in pair.test_forward_matches_rfft_of_windowed_frames.pytestmark
             if m.name == "parametrize"}
    for n in marks["n"]:
        for dtype in marks["dtype"]:
            for window in pair.WINDOWS + ["table"]:
                seen.add(forward_inst(n, dtype, window))
    logs, flags = range(5, 14), (False, True)
    full = {("istft_frame_kernel", d, L, w, x) for d in DTYPES for L in logs for w in flags for x in flags}
    full |= {("stft_complex_kernel", d, L, w, None) for d in DTYPES for L in logs for w in flags}
    full |= {("istft_ola_kernel", d, None, w, None) for d in DTYPES for w in flags}
    assert len(full) == 72 + 36 + 4
    missing = full - seen
    assert not missing, sorted(map(str, missing))
    assert seen == full, sorted(map(str, seen - full))
    # the a and b tables alone reach all of them too (the pair file's table only repeats the forward ones)
    print(f"STFTERR case=c kind=coverage reached={len(seen)} of={len(full)} share=0.000")


# ---- d ------------------------------------------------------------------------------------------------------------

D_SHAPES = [(64, 1, 200), (64, 3, 100), (128, 1, 300), (256, 5, 150), (512, 7, 200), (1024, 8, 300), (2048, 16, 300),
            (8192, 64, 260), (16384, 128, 300)]
D_COUNT_SHAPES = [(64, 3, 100), (256, 5, 150)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("shape", D_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_d_overlap_add_at_full_depth(plans, shape, dtype):
    n, hop, frames = shape
    plan = plans(n, dtype)
    rng = np.random.default_rng(n + hop + frames)
    k = math.ceil(n / hop) - 1
    assert frames > 2 * k + 3  # every chunk size below gives more than one chunk
    bins = n // 2 + 1
    re, im = gauss(rng, (frames, bins), dtype), gauss(rng, (frames, bins), dtype)
    spec = to_np(re) + 1j * to_np(im)
    t = Tally("d", "inverse", dtype, n)
    for window in ("rect", "hann"):
        first = istft_filled(plan, re, im, hop, window)
        got = to_np(first)
        want, den, ymax = ref_istft(spec, n, hop, win64(plan, window))
        assert got.shape == want.shape
        t.exact(zeros_where_den_small(got, den), (window, "zeros where den <= 1e-11"))
        t.add(inv_err(got, want, den, ymax, n, hop), INV_TOL[dtype], (window, hop, frames))
        prev = set_chunk(1)
        try:
            for s in (1, k, k + 1, 2 * k + 3):
                set_chunk(s)
                t.exact(torch.equal(istft_filled(plan, re, im, hop, window), first), (window, "chunk frames", s))
        finally:
            set_chunk(prev)
        if window == "rect" and shape in D_COUNT_SHAPES:
            # den is exactly the count of covering frames: out = (0 + y_b0 + y_b1 + ...) / count in ascending b, in the
            # output's precision, from the device's own frames (rect at hop = N: out = y_b / 1)
            y = plan.istft(re, im, n, "rect").cpu().numpy().reshape(frames, n)
            num, cnt = np.zeros(got.size, dtype=y.dtype), np.zeros(got.size, dtype=y.dtype)
            for b in range(frames):
                num[b * hop:b * hop + n] += y[b]
                cnt[b * hop:b * hop + n] += 1
            assert num.dtype == y.dtype and cnt.max() == k + 1
            t.exact(np.array_equal(first.cpu().numpy(), num / cnt), (window, "out * count = the ascending sum"))
    t.done()


# ---- e ------------------------------------------------------------------------------------------------------------

def default_chunk_frames(n, hop, itemsize):
    """S of include/pdsp_hip.h: max(K + 1, 2^28 bytes / (N sizeof T) - K), K = ceil(N / hop) - 1 (and one chunk's outputs
    within a 32-bit grid, which binds at neither case below)."""
    k = math.ceil(n / hop) - 1
    s = max(k + 1, (1 << 28) // (n * itemsize) - k)
    return min(s, (0x7fffffff - 2 * n) // hop), k


def region_ref(re, im, n, hop, w, a, b):
    """ref_istft of outputs [a, b), from only the frames that cover them: (want, den, max|y|)."""
    frames = re.shape[0]
    f0, f1 = max(0, -((n - 1 - a) // hop)), min(frames - 1, (b - 1) // hop)  # ceil((a - n + 1) / hop) ... (b - 1) // hop
    want, den, ymax = ref_istft(to_np(re[f0:f1 + 1]) + 1j * to_np(im[f0:f1 + 1]), n, hop, w)
    off = f0 * hop
    return want[a - off:b - off], den[a - off:b - off], ymax


@pytest.mark.parametrize("dtype,n,hop,extra", [(torch.float32, 16384, 4096, 40), (torch.float64, 64, 16, 1000)],
                         ids=["f32-16384", "f64-64"])
def test_e_default_chunk_boundary(plans, dtype, n, hop, extra):
    plan = plans(n, dtype)
    s, k = default_chunk_frames(n, hop, torch.empty((), dtype=dtype).element_size())
    frames, bins = s + extra, n // 2 + 1
    assert frames > s > 3 * (k + 1)
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(n + hop)
    re = torch.randn((frames, bins), generator=gen, dtype=dtype, device="cuda:0")
    im = torch.randn((frames, bins), generator=gen, dtype=dtype, device="cuda:0")
    t = Tally("e", "inverse", dtype, n)
    prev = set_chunk(0)
    try:
        out = istft_filled(plan, re, im, hop, "hann")  # the default S: two chunks
        set_chunk(s // 3)
        t.exact(torch.equal(istft_filled(plan, re, im, hop, "hann"), out), ("chunk frames", s // 3))
    finally:
        set_chunk(prev)
    total = (frames - 1) * hop + n
    assert out.shape == (total,)
    w = win64(plan, "hann")
    for a, b in ((0, n), (s * hop - n, s * hop + n), (total - n, total)):
        want, den, ymax = region_ref(re, im, n, hop, w, a, b)
        got = to_np(out[a:b])
        t.exact(zeros_where_den_small(got, den), (a, b, "zeros where den <= 1e-11"))
        t.add(inv_err(got, want, den, ymax, n, hop), INV_TOL[dtype], (a, b))
    del re, im, out
    torch.cuda.empty_cache()
    t.done()


# ---- f ------------------------------------------------------------------------------------------------------------

def f_shapes(n):
    r = rows_per_wg(n)
    if r > 1:
        shapes = [(f, h) for f in (1, 2) for h in (n // 4 + 1, n + 3)]
        shapes += [(f, h) for f in (r - 1, r + 1, 2 * r + 1) for h in (n // 2, n)]
    else:
        shapes = [(f, h) for f in (1, 2, 3) for h in (n // 4 + 1, n + 3, n // 2, n)]
    return sorted(set(shapes))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", SIZES)
def test_f_few_frames_and_dead_rows(plans, n, dtype):
    plan = plans(n, dtype)
    rng = np.random.default_rng(11 * n + SFX[dtype].count("6"))
    bins = n // 2 + 1
    t = Tally("f", "inverse", dtype, n)
    for frames, hop in f_shapes(n):
        re, im = gauss(rng, (frames, bins), dtype), gauss(rng, (frames, bins), dtype)
        spec = to_np(re) + 1j * to_np(im)
        total = (frames - 1) * hop + n
        for window in ("rect", "hann"):
            buf = torch.full((total + 2 * GUARD,), NAN, dtype=dtype, device="cuda:0")
            raw_istft(plan, dtype, frames, re, im, hop, win_arg(plan, window), buf[GUARD:])
            torch.cuda.synchronize()
            t.exact(bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + total:]).all()),
                    (frames, hop, window, "margins"))
            got = to_np(buf[GUARD:GUARD + total])
            want, den, ymax = ref_istft(spec, n, hop, win64(plan, window))
            t.exact(zeros_where_den_small(got, den), (frames, hop, window, "zeros where den <= 1e-11"))
            t.add(inv_err(got, want, den, ymax, n, hop), INV_TOL[dtype], (frames, hop, window))
    t.done()


# ---- g ------------------------------------------------------------------------------------------------------------

def off_boundary(count, dtype, src=None):
    """`count` elements that start one element past a 16-byte boundary inside a NaN-filled buffer: (buffer, view)."""
    buf = torch.full((2 * GUARD + 1 + count,), NAN, dtype=dtype, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    view = buf[GUARD + 1:GUARD + 1 + count]
    assert view.data_ptr() % 16 == view.element_size()
    if src is not None:
        view.copy_(src.reshape(-1))
    return buf, view


def margins_intact(buf, count):
    return bool(torch.isnan(buf[:GUARD + 1]).all() and torch.isnan(buf[GUARD + 1 + count:]).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [64, 512, 16384])
def test_g_misaligned_bases(plans, n, dtype):
    plan = plans(n, dtype)
    rng = np.random.default_rng(13 * n + SFX[dtype].count("6"))
    frames, bins = 7, n // 2 + 1
    table = table_window(rng, n, dtype)
    assert table.data_ptr() % 16 == 0
    t = Tally("g", "bits", dtype, n)
    for hop in (n // 4 + 1, n):
        # forward: signal, window table, re_out, im_out
        x = gauss(rng, n + (frames - 1) * hop, dtype)
        re, im = plan.stft_complex(x, hop, table)
        assert x.data_ptr() % 16 == re.data_ptr() % 16 == im.data_ptr() % 16 == 0
        bufs = [off_boundary(x.numel(), dtype, x), off_boundary(n, dtype, table), off_boundary(frames * bins, dtype),
                off_boundary(frames * bins, dtype)]
        (_, ox), (_, ow), (_, ore), (_, oim) = bufs
        raw_stft(plan, dtype, frames, ox, n, hop, ow, ore, oim)
        torch.cuda.synchronize()
        t.exact(torch.equal(ore.reshape(frames, bins), re) and torch.equal(oim.reshape(frames, bins), im),
                (hop, "forward bits"))
        t.exact(all(margins_intact(b, v.numel()) for b, v in bufs), (hop, "forward margins"))
        # inverse: re_in, im_in, window, out
        out = plan.istft(re, im, hop, table)
        assert out.data_ptr() % 16 == 0
        bufs = [off_boundary(frames * bins, dtype, re), off_boundary(frames * bins, dtype, im),
                off_boundary(n, dtype, table), off_boundary(out.numel(), dtype)]
        (_, ire), (_, iim), (_, iw), (_, oout) = bufs
        raw_istft(plan, dtype, frames, ire, iim, hop, iw, oout)
        torch.cuda.synchronize()
        t.exact(torch.equal(oout, out), (hop, "inverse bits"))
        t.exact(all(margins_intact(b, v.numel()) for b, v in bufs), (hop, "inverse margins"))
    t.done()


# ---- h ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [64, 1024, 8192])
def test_h_imaginary_parts_of_bins_0_and_half_are_ignored(plans, n, dtype):
    plan = plans(n, dtype)
    rng = np.random.default_rng(17 * n + SFX[dtype].count("6"))
    frames, bins = 9, n // 2 + 1
    re, im = gauss(rng, (frames, bins), dtype), gauss(rng, (frames, bins), dtype)
    clean, dirty = im.clone(), im.clone()
    clean[:, 0] = 0
    clean[:, -1] = 0
    junk = torch.tensor([NAN, float("inf"), float("-inf")], dtype=dtype, device="cuda:0")
    dirty[:, 0] = junk[torch.arange(frames) % 3]
    dirty[:, -1] = junk[(torch.arange(frames) + 1) % 3]
    t = Tally("h", "bits", dtype, n)
    for hop in (n // 2, n):
        for window in ("rect", "hann"):
            want = plan.istft(re, clean, hop, window)
            t.exact(bool(torch.isfinite(want).all()), (hop, window, "finite"))
            t.exact(torch.equal(plan.istft(re, dirty, hop, window), want), (hop, window, "non-finite = zeros"))
            t.exact(torch.equal(plan.istft(re, im, hop, window), want), (hop, window, "finite = zeros"))
    t.done()


# ---- i ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", [64, 4096])
def test_i_non_finite_values_stay_local(plans, n, dtype):
    plan = plans(n, dtype)
    rng = np.random.default_rng(19 * n + SFX[dtype].count("6"))
    frames, bins = 9, n // 2 + 1
    table = table_window(rng, n, dtype)  # strictly positive
    t = Tally("i", "bits", dtype, n)
    for hop in (n // 4 + 1, n + 3):
        # forward: a NaN at sample p, an Inf at sample q (the last sample of frame 5)
        x = gauss(rng, n + (frames - 1) * hop, dtype)
        p, q = 3 * hop + 1, 5 * hop + n - 1
        bad = x.clone()
        bad[p], bad[q] = NAN, float("inf")
        hit = [any(b * hop <= s < b * hop + n for s in (p, q)) for b in range(frames)]
        assert 2 <= sum(hit) < frames
        for window in ("rect", table):
            wname = window if isinstance(window, str) else "table"
            re, im = plan.stft_complex(x, hop, window)
            bre, bim = plan.stft_complex(bad, hop, window)
            t.exact(bool(torch.isfinite(re).all() and torch.isfinite(im).all()), (hop, wname, "forward clean finite"))
            for b in range(frames):
                if hit[b]:
                    t.exact(not bool(torch.isfinite(bre[b]).all() and torch.isfinite(bim[b]).all()),
                            (hop, wname, b, "covering frame is non-finite"))
                else:
                    t.exact(torch.equal(bre[b], re[b]) and torch.equal(bim[b], im[b]), (hop, wname, b, "other frame's bits"))
        # inverse: a NaN in one bin of frame 3
        re, im = gauss(rng, (frames, bins), dtype), gauss(rng, (frames, bins), dtype)
        bad = re.clone()
        bad[3, 5] = NAN
        clean = plan.istft(re, im, hop, table)
        out = plan.istft(bad, im, hop, table)
        inside = torch.zeros(out.numel(), dtype=torch.bool, device="cuda:0")
        inside[3 * hop:3 * hop + n] = True
        t.exact(bool(torch.isfinite(clean).all()), (hop, "inverse clean finite"))
        t.exact(bool((~torch.isfinite(out[inside])).all()), (hop, "every sample of the frame is non-finite"))
        t.exact(torch.equal(out[~inside], clean[~inside]), (hop, "other samples' bits"))
    t.done()


# ---- j ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n,hop", [(256, 64), (1024, 333), (4096, 4096)])
def test_j_inverse_agrees_with_torch_istft(plans, n, hop, dtype):
    """torch.istft on CPU tensors of the case's dtype (no hipFFT); the other implementation gets the factor 2 that the
    pair file's torch.stft comparison gives it."""
    plan = plans(n, dtype)
    rng = np.random.default_rng(23 * n + SFX[dtype].count("6"))
    frames, bins = 7, n // 2 + 1
    re = torch.from_numpy(rng.standard_normal((frames, bins))).to(dtype)
    im = torch.from_numpy(rng.standard_normal((frames, bins))).to(dtype)
    im[:, 0] = 0
    im[:, -1] = 0
    t = Tally("j", "inverse-vs-torch", dtype, n)
    for window in ("hamming", table_window(rng, n, dtype)):
        wname = window if isinstance(window, str) else "table"
        w = win64(plan, window)
        want = torch.istft(torch.complex(re, im).t().contiguous(), n_fft=n, hop_length=hop, win_length=n,
                           window=torch.from_numpy(w).to(dtype), center=False, onesided=True, return_complex=False)
        assert want.dtype == dtype
        got = to_np(plan.istft(re.cuda(), im.cuda(), hop, window))
        assert got.shape == tuple(want.shape)
        _, den, ymax = ref_istft(to_np(re) + 1j * to_np(im), n, hop, w)
        t.add(inv_err(got, to_np(want), den, ymax, n, hop), 2 * INV_TOL[dtype], (wname, hop))
    t.done()


# ---- k ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("n", SIZES)
def test_k_round_trip_at_every_size(plans, n, dtype):
    plan = plans(n, dtype)
    rng = np.random.default_rng(29 * n + SFX[dtype].count("6"))
    t = Tally("k", "round-trip", dtype, n)
    for hop in (n // 4, n // 3 + 1):
        for window in ("hann", "hamming"):
            x = gauss(rng, n + 8 * hop, dtype)
            re, im = plan.stft_complex(x, hop, window)
            assert re.shape[0] == 9
            out = to_np(plan.istft(re, im, hop, window))
            _, den, _ = ref_istft(np.zeros((re.shape[0], n // 2 + 1)), n, hop, win64(plan, window))
            x64 = to_np(x)[:out.size]
            ok = den > THR * (1 + 1e-4)
            err = (np.abs(out - x64)[ok] * np.sqrt(den[ok])).max() / (np.abs(x64).max() * math.sqrt(math.ceil(n / hop)))
            t.add(err, RT_TOL[dtype], (hop, window))
            t.exact(bool(np.all(out[den <= THR * (1 - 1e-4)] == 0.0)), (hop, window, "zeros where den <= 1e-11"))
    t.done()


# ---- l ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [128, 512, 8192])
def test_l_python_host_forms(plans, n):
    """pragma_dsp_amd.stft / istft (numpy in, numpy out, f64 on the device) against the references at the f64 bounds,
    and bit for bit against BatchedFft(n, torch.float64) on the same data."""
    import pragma_dsp_amd as pd
    dtype = torch.float64
    plan = plans(n, dtype)
    rng = np.random.default_rng(31 * n)
    frames, bins = 7, n // 2 + 1
    tf, ti = Tally("l", "forward", dtype, n), Tally("l", "inverse", dtype, n)
    for hop in (n // 4 + 1, n):
        x = rng.standard_normal(n + (frames - 1) * hop + (hop - 1))  # the tail shorter than a hop is ignored
        spec = rng.standard_normal((frames, bins)) + 1j * rng.standard_normal((frames, bins))
        for window in pair.WINDOWS:
            w = win64(plan, window)
            got = pd.stft(x, n, hop, window)
            assert got.shape == (frames, bins) and got.dtype == np.complex128
            want = ref_stft(x, n, hop, w)
            tf.add(np.abs(got - want).max() / np.abs(want).max(), FWD_TOL[dtype], (hop, window))
            re, im = plan.stft_complex(torch.from_numpy(x).cuda(), hop, window)
            tf.exact(np.array_equal(got.real, re.cpu().numpy()) and np.array_equal(got.imag, im.cpu().numpy()),
                     (hop, window, "host form = BatchedFft bits"))
            out = pd.istft(spec, hop, window)
            want, den, ymax = ref_istft(spec, n, hop, w)
            assert out.shape == want.shape and out.dtype == np.float64
            ti.exact(zeros_where_den_small(out, den), (hop, window, "zeros where den <= 1e-11"))
            ti.add(inv_err(out, want, den, ymax, n, hop), INV_TOL[dtype], (hop, window))
            dev = plan.istft(torch.from_numpy(spec.real.copy()).cuda(), torch.from_numpy(spec.imag.copy()).cuda(), hop, window)
            ti.exact(np.array_equal(out, dev.cpu().numpy()), (hop, window, "host form = BatchedFft bits"))
    try:
        tf.done()
    finally:
        ti.done()

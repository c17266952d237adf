"""Every row family that came after the FFT, spectrum and FIR kernels at machine-filling batches, bit for bit: DCT-II /
-III, Hilbert (analytic, envelope), FIR overlap-save, STFT / ISTFT, the any-length DFT, the chirp-z transform, the DWT
(resident and tiled, both directions), polyphase resampling, the sliding DFT, and the NTT with its exact convolution.

Their own modules check "a row's output depends on the row alone" with a handful of rows, one to three workgroups.
Here K = 61 seeded base rows are run once as a 61-row call, whose result is held to the family's own reference, metric
and bound (all three imported from the family's test module; no tolerance is introduced here), and then tiled on the
device to B rows, row r = base row r mod 61, with B chosen so that the launch has at least W = 32 x CUs workgroups --
at least four complete rounds of workgroups replacing each other on every CU (tests/full_machine_cases.py says why, and
holds the table and the batch arithmetic, which tests/test_full_machine_cases_cpu.py checks without a GPU).  Every group
of 61 output rows must equal the 61-row result, and the remainder its first rows, on the bit patterns, compared on the
device in slices of at most 2^28 elements; a second identical launch must give the same bits.

  test_rows_do_not_depend_on_the_batch   the table: the smallest row shapes that reach each distinct geometry
  test_rows_past_the_byte_lines          DCT, FIR, DWT, upfirdn at their largest row with f64 planes past 2^32 bytes
                                         and, at the same B, f32 planes past 2^31
  test_layouts_at_the_middle_shape       one launch each: the exact in-place call; rows at strides that are multiples
                                         of 16 bytes (FAST where the family has one); rows at odd strides behind a
                                         one-element offset (the general path) -- NaN in every gap and guard band,
                                         untouched afterwards

STFT frames come from one long signal whose period is 61 hops; the ISTFT's spectra are frame-periodic, and every
interior output period of 61 hops is compared with the same period of a short run of 3 x 61 + ceil(N / hop) frames (up
to 2 N samples at each end are left out: the window-sum normalisation differs there).  The f64 N = 16384 ISTFT runs at
the default chunking, at least four chunks of 256 MiB of scratch.

At M = 8192 the chirp-z reference is computed for three of the 61 rows, as tests/test_gpu_czt.py does for its 37; at
N = 2^14 the NTT's Python-integer reference for three, as tests/test_gpu_ntt.py runs three-row batches from N = 4096 on.

Every case prints one FULLMACHINE line: family, shape, dtype, rows, workgroups, bytes in and out, seconds.  On a
mismatch the assertion names the first differing row, its base row, workgroup, slot within the workgroup, column and
both bit patterns: the same slot in every workgroup points at LDS slicing, late workgroups only at residency or
in-place ordering, rows beyond a byte line only at addressing, chunk seams only at the ISTFT's chunk loop."""
import functools
import math
import time
from types import SimpleNamespace

import numpy as np
import pytest

import full_machine_cases as FM
import ntt_ref
import sdft_ref as R
import test_gpu_czt as CZT
import test_gpu_dct as DCT
import test_gpu_dft as DFT
import test_gpu_dwt as DWT
import test_gpu_fir_paths as FIR
import test_gpu_hilbert as HIL
import test_gpu_ntt as NTT
import test_gpu_resample as RES
import test_gpu_resample_paths as RESP
import test_gpu_row_invariances as INV
import test_gpu_stft_pair as STFT
from test_czt_cpu import GRID, grid_direct
from test_czt_cpu import row_err as czt_row_err
from test_dct_cpu import dct_ref
from test_dft_cpu import row_err as dft_row_err
from test_hilbert_cpu import hilbert_ref
from test_resample_cpu import user_taps

pytestmark = pytest.mark.gpu

K = FM.K
NAN = float("nan")


def lg2(n):
    return n.bit_length() - 1


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- the families: inputs (K base rows per plane, on the device), run(xs, out) -> the output planes, hold(ref) -------------

def build_dct(c):
    n, = c.shape
    p = HIL.plan(None, n, c.dt)
    x = INV.gauss(7 * n + c.op, (K, n), c.dt)

    def hold(ref):
        e = DCT.rel_rows(host(ref[0]), dct_ref(x, c.op, "backward"))
        assert e <= DCT.TOL[c.dt] * lg2(n), (FM.case_id(c), e)
    return SimpleNamespace(inputs=(INV.dev(x, c.dt),), hold=hold, fast=lambda xs, ys: DCT._fast(xs[0], ys[0]),
                           run=lambda xs, out=None: (p.dct(xs[0], type=c.op, out=out and out[0]),))


def build_hilbert(c):
    n, = c.shape
    p = HIL.plan(None, n, c.dt)
    x = INV.gauss(11 * n, (K, n), c.dt)

    def hold(ref):
        e = HIL.err_rows(host(ref[0]), hilbert_ref(x), c.op)
        assert e <= HIL.bound(c.dt, n, c.op), (FM.case_id(c), e)
    return SimpleNamespace(inputs=(INV.dev(x, c.dt),), hold=hold, fast=lambda xs, ys: HIL._fast(p, xs[0], ys[0], c.op),
                           run=lambda xs, out=None: (HIL.run(p, xs[0], c.op, out=out and out[0]),))


def build_fir(c):
    import pragma_dsp_amd as pd
    n, = c.shape
    ntaps, length = FM.fir_shape(n)
    h = INV.gauss(13 * n, ntaps, c.dt)
    x = INV.gauss(13 * n + 1, (K, length), c.dt)
    f = pd.FirFilter(h, "cuda:0", INV.tdt(c.dt), block=n)

    def hold(ref):
        assert tuple(ref[0].shape) == (K, length)
        e = FIR.err(host(ref[0]), FIR.f64_full(x, h)[:, :length], x, h)  # "filter": the first len outputs
        assert e <= FIR.tol(c.dt, n, FIR.TOL_GAUSS), (FM.case_id(c), e)

    def fast(xs, ys):
        return FIR._fast(xs[0].data_ptr(), ys[0].data_ptr(), xs[0].stride(0), ys[0].stride(0), n, ntaps, 0)
    return SimpleNamespace(inputs=(INV.dev(x, c.dt),), hold=hold, fast=fast,
                           run=lambda xs, out=None: (f.apply(xs[0], "filter", out=out and out[0]),))


def build_stft(c):
    import torch
    n, hop = c.shape
    p = HIL.plan(None, n, c.dt)
    base = INV.gauss(17 * n + hop, (K, hop), c.dt)

    def tile(xs, frames):  # one signal whose period is 61 hops: frame f + 61 is frame f
        idx = torch.arange(frames - 1 + n // hop, device="cuda") % K
        return (xs[0].index_select(0, idx).reshape(-1),)

    def hold(ref):
        want = STFT.ref_stft(FM.periodic_signal(base, K, n), n, hop, STFT.win64(p, "hann"))
        got = host(ref[0]).astype(np.float64) + 1j * host(ref[1]).astype(np.float64)
        e = np.abs(got - want).max() / np.abs(want).max()  # the metric of test_forward_matches_rfft_of_windowed_frames
        assert e <= STFT.FWD_TOL[INV.tdt(c.dt)] * math.log2(n), (FM.case_id(c), e)
    return SimpleNamespace(inputs=(INV.dev(base, c.dt),), hold=hold, tile=tile,
                           run=lambda xs, out=None: p.stft_complex(xs[0], hop, "hann"))


def build_istft(c):
    n, hop = c.shape
    p = HIL.plan(None, n, c.dt)
    z = INV.gauss(19 * n + hop, (2, K, n // 2 + 1), c.dt)
    short = 3 * K + -(-n // hop)

    def rows_view(outs, frames):
        """The interior of the output as rows of one hop, from sample 61 hop (>= 2 N) to 2 N before the end."""
        total = (frames - 1) * hop + n
        assert outs[0].shape == (total,) and K * hop >= 2 * n
        rows = (total - 2 * n - K * hop) // hop
        return [outs[0][K * hop:(K + rows) * hop].view(rows, hop)]

    def hold(ref):
        idx = np.arange(short) % K
        want, den, ymax = STFT.ref_istft(z[0][idx] + 1j * z[1][idx], n, hop, STFT.win64(p, "hann"))
        got = host(ref[0]).astype(np.float64)
        assert got.shape == want.shape
        # the metric of test_inverse_matches_the_definition
        zero = (den <= STFT.THR) & (np.abs(den - STFT.THR) > 1e-4 * STFT.THR)
        assert np.all(got[zero] == 0.0)
        good = den >= 1e-3 * den.max()
        e = (np.abs(got - want)[good] * np.sqrt(den[good])).max() / (ymax * math.sqrt(math.ceil(n / hop)))
        assert e <= STFT.INV_TOL[INV.tdt(c.dt)] * math.log2(n), (FM.case_id(c), e)
    return SimpleNamespace(inputs=(INV.dev(z[0], c.dt), INV.dev(z[1], c.dt)), hold=hold, ref_rows=short,
                           rows_view=rows_view, ref_view=lambda outs: [outs[0][K * hop:2 * K * hop].view(K, hop)],
                           run=lambda xs, out=None: (p.istft(xs[0], xs[1], hop, "hann"),))


def build_dft(c):
    ln, = c.shape
    d = DFT.dft_of(ln)
    re, im, z = DFT.gauss(1000 * ln + (c.dt == "f64"), K, ln, c.dt)

    def hold(ref):
        e = dft_row_err(DFT.cplx(ref), (np.fft.fft if c.op == "forward" else np.fft.ifft)(z))
        assert e <= DFT.bound(c.dt, ln), (FM.case_id(c), e)
    return SimpleNamespace(inputs=(re, im), hold=hold,
                           run=lambda xs, out=None: getattr(d, c.op)(xs[0], xs[1], out=out))


@functools.lru_cache(maxsize=None)
def czt_reference(ln, bins, dt):
    _, _, z = DFT.gauss(1000 * ln + 2 * bins + (dt == "f64"), K, ln, dt)
    rows = [0, K // 2, K - 1] if FM.conv_size(ln + bins - 1) == 8192 else list(range(K))
    return rows, z, grid_direct(z[rows], bins, CZT.P, CZT.Q, 1.0, extended=(dt == "f64"))


def build_czt(c):
    ln, bins = c.shape
    t = CZT.czt_of(ln, bins, CZT.P / GRID, CZT.Q / GRID, 1.0)
    re, im, _ = DFT.gauss(1000 * ln + 2 * bins + (c.dt == "f64"), K, ln, c.dt)

    def hold(ref):
        rows, z, want = czt_reference(ln, bins, c.dt)
        e = czt_row_err(DFT.cplx(ref)[rows], want, z[rows], 1.0)
        assert e <= CZT.bound(c.dt, ln, bins), (FM.case_id(c), e)
    return SimpleNamespace(inputs=(re, im), hold=hold, run=lambda xs, out=None: t.forward(xs[0], xs[1], out=out))


def build_dwt(c):
    n, levels, key = c.shape
    tdt = INV.tdt(c.dt)
    cs = DWT.case(n, levels, key, tdt, K)
    w = INV.dwt_handle(key, levels, c.dt)
    assert w.ntaps == FM.DWT_TAPS[key]
    src, want, bound = (cs["x"], cs["fwd"], cs["fwd_bound"]) if c.op == "forward" else (cs["c"], cs["inv"], cs["inv_bound"])
    return SimpleNamespace(inputs=(DWT.dev(src, tdt),),
                           hold=lambda ref: DWT.hold(DWT.host(ref[0]), want, bound, FM.case_id(c)),
                           run=lambda xs, out=None: (getattr(w, c.op)(xs[0], out=out and out[0]),))


def build_upfirdn(c):
    import pragma_dsp_amd as pd
    up, down, ntaps, n = c.shape
    tdt = INV.tdt(c.dt)
    r = pd.Upfirdn(user_taps(ntaps), up, down, device="cuda:0", dtype=tdt)
    assert r.output_len(n) == FM.upfirdn_output_len(n, up, down, ntaps)
    x = RES.signal((K, n), tdt, 1000 * up + ntaps)
    return SimpleNamespace(inputs=(RES.dev(x, tdt),),
                           hold=lambda ref: RESP.hold(ref[0], x, up, down, r.taps, 0, tdt, FM.case_id(c)),
                           run=lambda xs, out=None: (r.apply(xs[0], out=out and out[0]),))


@functools.lru_cache(maxsize=None)
def sdft_reference(n, t, hop, win):
    x = np.random.default_rng([n, t, 0]).standard_normal((K, t)).astype(np.float32).astype(np.float64)  # sdft_ref.signal
    fr = R.pick_frames(n, hop, t)
    return x, fr, R.direct(x, n, R.path_bins(n), hop, win, fr)


def build_sdft(c):
    import pragma_dsp_amd as pd
    n, t, hop, win = c.shape
    assert len(R.path_bins(n)) == FM.SDFT_BINS
    s = pd.SlidingDft(n, list(R.path_bins(n)), hop=hop, window=win)
    x, fr, (re, im) = sdft_reference(n, t, hop, win)

    def hold(ref):
        got = host(ref[0]).astype(np.float64) + 1j * host(ref[1]).astype(np.float64)
        assert got.shape == (K, FM.SDFT_BINS, R.frames_of(n, hop, t))
        e = R.err_units(got[:, :, fr], re, im, n, c.dt, np.abs(x).max())
        assert e <= R.BOUND[c.dt], (FM.case_id(c), e)
    return SimpleNamespace(inputs=(INV.dev(x, c.dt),), hold=hold, run=lambda xs, out=None: s.forward(xs[0]))


def build_ntt(c):
    import pragma_dsp_amd as pd
    import torch
    lg, = c.shape
    n = 1 << lg
    plan = pd.Ntt(n, "cuda:0")
    a = ntt_ref.rows(n, K, 0)
    b = ntt_ref.rows(n, K, 3, seed=1)
    rows = list(range(K)) if lg < 12 else [0, K // 2, K - 1]
    if c.op == "convolve":
        inputs = (NTT.dev(a, torch.int64), NTT.dev(b, torch.int64))

        def run(xs, out=None):
            return (plan.convolve(xs[0], xs[1], out_len=n, out=out and out[0]),)
    else:
        inputs = (NTT.dev(a, torch.int64),)

        def run(xs, out=None):
            return (getattr(plan, c.op)(xs[0], out=out and out[0]),)

    def hold(ref):
        got = NTT.host(ref[0][rows])
        if c.op == "convolve":
            assert got == [ntt_ref.cyclic(a[i], b[i], n) for i in rows], FM.case_id(c)
        else:
            assert got == ntt_ref.transform_rows([a[i] for i in rows], inverse=c.op == "inverse"), FM.case_id(c)
    return SimpleNamespace(inputs=inputs, hold=hold, run=run)


BUILD = {"dct": build_dct, "hilbert": build_hilbert, "fir": build_fir, "stft": build_stft, "istft": build_istft,
         "dft": build_dft, "czt": build_czt, "dwt": build_dwt, "upfirdn": build_upfirdn, "sdft": build_sdft,
         "ntt": build_ntt}


# ---- the harness ------------------------------------------------------------------------------------------------------

def bits(t):
    """A real, complex or 64-bit integer tensor [rows, ...] as a 2-D tensor of its bit patterns (a view)."""
    import torch
    if t.is_complex():
        t = torch.view_as_real(t)
    t = t.view(torch.int32 if t.element_size() == 4 else torch.int64)
    return t if t.dim() == 2 else t.flatten(1)


def tile_rows(xs, b):
    import torch
    idx = torch.arange(b, device="cuda") % K
    return tuple(x.index_select(0, idx) for x in xs)


def padded(like, rows, stride, off):
    """(the buffer as real values, all NaN; a [rows, like.shape[1]] view of like's dtype at row stride `stride`, `off`
    elements in) -- eight elements of guard band behind the last row."""
    import torch
    k = 2 if like.is_complex() else 1
    rdt = torch.float32 if like.element_size() // k == 4 else torch.float64
    real = torch.full((k * (off + rows * stride + 8),), NAN, dtype=rdt, device="cuda")
    buf = torch.view_as_complex(real.view(-1, 2)) if k == 2 else real
    return real, buf.as_strided((rows, like.shape[1]), (stride, 1), off)


def untouched(real, view):
    """Every value of the buffer outside the view's rows is still NaN, and no value inside is."""
    import torch
    k = 2 if view.is_complex() else 1
    inside = view.shape[0] * view.shape[1] * k
    return int(torch.isnan(real).sum()) == real.numel() - inside and not bool(torch.isnan(view).any())


def compare(c, fam, outs, ref_bits, b, what):
    views = fam.rows_view(outs, b) if hasattr(fam, "rows_view") else list(outs)
    assert len(views) == len(ref_bits)
    for plane, (v, rb) in enumerate(zip(views, ref_bits)):
        if not hasattr(fam, "rows_view"):
            assert v.shape[0] == b, (FM.case_id(c), what, tuple(v.shape))
        bad = FM.first_mismatch(bits(v), rb)
        assert bad is None, f"{FM.case_id(c)} {what}, output plane {plane}: " + FM.describe(c, *bad)


def full_machine(c):
    """One case; whatever it leaves on the device is freed before the next one, whether it passed or not."""
    import gc

    import torch
    try:
        run_case(c)
    finally:
        gc.collect()
        torch.cuda.empty_cache()


def run_case(c):
    import torch
    t0 = time.perf_counter()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    b = FM.rows_of(c, cus)
    wgs = FM.workgroups(c, b)
    bin_, bout = FM.bytes_in_out(c, b)
    assert wgs >= FM.ROUNDS * cus and FM.live_bytes(c, b) <= FM.LIVE_LIMIT
    fam = BUILD[c.family](c)
    tile = getattr(fam, "tile", tile_rows)

    # the 61-row call (ISTFT: the short run), held to the family's reference at the family's bound
    ref = fam.run(tile(fam.inputs, getattr(fam, "ref_rows", K)))
    fam.hold(ref)
    ref_bits = [bits(v).contiguous() for v in (fam.ref_view(ref) if hasattr(fam, "ref_view") else ref)]
    assert all(r.shape[0] == K for r in ref_bits)

    xs = tile(fam.inputs, b)
    if c.variant is None:
        for launch in ("first launch", "second launch"):
            outs = fam.run(xs)
            compare(c, fam, outs, ref_bits, b, launch)
            del outs
    elif c.variant == "inplace":
        outs = fam.run(xs, out=xs)
        assert all(o.data_ptr() == x.data_ptr() for o, x in zip(outs, xs))
        compare(c, fam, outs, ref_bits, b, "in place")
        del outs
    else:
        off = 1 if c.variant == "odd" else 0
        xin, youts = [], []
        for x in xs:
            xin.append(padded(x, b, FM.stride_of(c, x.shape[1]), off))
            xin[-1][1].copy_(x)
        del xs
        for r in ref:
            youts.append(padded(r, b, FM.stride_of(c, r.shape[1]), off))
        xs = tuple(v for _, v in xin)
        outs = fam.run(xs, out=tuple(v for _, v in youts))
        for x in xs + tuple(outs):  # the layouts are what they are called
            if c.variant == "fast":
                assert (x.stride(0) * x.element_size()) % 16 == 0 and x.data_ptr() % 16 == 0
            else:
                assert x.stride(0) % 2 == 1 and x.storage_offset() == 1
        if hasattr(fam, "fast"):
            assert fam.fast(xs, outs) == (c.variant == "fast"), FM.case_id(c)
        compare(c, fam, outs, ref_bits, b, c.variant + " strides")
        for real, v in xin + youts:
            assert untouched(real, v), (FM.case_id(c), "a sentinel was overwritten")
        del outs, xin, youts
    torch.cuda.synchronize()
    shape = "x".join(str(v) for v in c.shape)
    print(f"FULLMACHINE {c.family} op={c.op} shape={shape} {c.dt} variant={c.variant} rows={b} workgroups={wgs} "
          f"(W={FM.ROUNDS * cus}) bytes_in={bin_} bytes_out={bout} seconds={time.perf_counter() - t0:.2f}")


def test_the_comparison_sees_one_flipped_bit_on_the_device():
    """The comparison itself, on a real output: one bit flipped in the last row of a full-machine DCT batch is found
    and named, and the untouched output passes."""
    import torch
    c = FM.Case("dct", 2, "f32", (64,), None, False)
    b = FM.rows_of(c, torch.cuda.get_device_properties(0).multi_processor_count)
    fam = build_dct(c)
    ref_bits = bits(fam.run(fam.inputs)[0]).contiguous()
    out = bits(fam.run(tile_rows(fam.inputs, b))[0])
    assert FM.first_mismatch(out, ref_bits) is None
    out[b - 1, 63] ^= 1
    row, col, got, want = FM.first_mismatch(out, ref_bits)
    assert (row, col, got ^ want) == (b - 1, 63, 1) and want == int(ref_bits[(b - 1) % K, 63])
    assert f"row {b - 1} (base row {(b - 1) % K}), workgroup {(b - 1) // 128}, slot {(b - 1) % 128}, column 63" \
        in FM.describe(c, row, col, got, want)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("case", FM.PLAIN, ids=FM.case_id)
def test_rows_do_not_depend_on_the_batch(case):
    full_machine(case)


@pytest.mark.parametrize("case", FM.LINES, ids=FM.case_id)
def test_rows_past_the_byte_lines(case):
    full_machine(case)


@pytest.mark.parametrize("case", FM.VARIANTS, ids=FM.case_id)
def test_layouts_at_the_middle_shape(case):
    full_machine(case)

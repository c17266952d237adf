"""Exact 2^k scaling, range edges and position independence of the row families that came after the FFT, spectrum and
FIR kernels: DCT-II / -III, Hilbert (four modes), STFT / ISTFT, the any-length DFT, the chirp-z transform, the DWT,
polyphase resampling and the sliding DFT.  Their own test modules hold them to accuracy bounds on Gaussian rows of unit
scale; this one asks what tests/test_gpu_f32_paths.py, test_gpu_f64_paths.py and test_gpu_fir_paths.py ask of the older
families.  Every reference, metric and bound is the family's own, imported from its test module.

(a) Exact scaling: out(2^k x) == 2^k out(x) bit for bit, k = -20 and 17 (the FFT tests' values).  Every operation of
    these kernels is a multiplication by a constant or an addition, so away from overflow and the subnormals scaling
    by a power of two commutes with every rounding: an equality, not a tolerance.  Rows: Gaussian, one impulse, one
    constant.  The Hilbert PHASE is scale-invariant, not scale-linear, and atan2 is the math library's: it is held to
    the reference at its bound.  (a) guards LINEARITY ONLY: a kernel that multiplies by g at another point, or that
    squares and takes a root with exact scaling, passes it at any k that stays in range.  Range is (b)'s job.
    Two places where a value is an f32 subnormal, so that the premise fails and not the kernel, are named where they
    are tested and held to the family's bound instead: SlidingDft at N = 2 on the constant row, and the f32 ENVELOPE
    on samples below its stated range.

(b) Range edges: the family's accuracy test again (Gaussian rows rounded to the dtype, its reference computed on the
    scaled inputs, its metric, its bound) on rows scaled by 2^k_hi and 2^k_lo, and every output finite.  With
    emax = 127 / 1023, emin = -126 / -1022, p = 24 / 53 (f32 / f64) and S the points of the family's transform (N; the
    convolution size M for Dft / Czt; the row length for DWT / upfirdn / SDFT; log2 S rounded up):

        k_hi = emax - log2 S - 4      one transform grows a row by at most its l1 norm, S max|x|; Gaussian rows of
                                      these sizes have max|x| < 2^2.2, which leaves more than a binade below 2^(emax+1)
                                      in the worst case and far more on these rows;
        k_hi = emax - 2 log2 M - 4    Dft / Czt: two transforms of M points with a product of modulus <= 1 in between
                                      and no 1 / M until the filter table;
        k_lo = emin + p + 2 log2 S + 4   at most S^2 roundings at the subnormal floor, each below 2^emin (a flushed
                                      value) or 2^(emin - p + 1) (a kept one), sum to S^2 2^emin = 2^(k_lo - p - 4)
                                      <= eps max|y| / 16, whether the target flushes subnormals or not.

    At N = 16384 this is k_lo = -70 in f32, far below 2^-63 where an f32 square leaves the normal range, and -937 in
    f64, below 2^-511; k_hi = 109 and 1005 are as far above 2^64 and 2^512.  Both ends expose any squaring of data.
    All the metrics are relative to a row's maximum (or to a sum of absolute terms that scales with the row), so they
    are homogeneous of degree 0; they are evaluated on got 2^-k and ref 2^-k, exact scalings, so that a norm inside a
    metric (test_czt_cpu.row_err squares the row) cannot leave f64's range.  The references alone were first run on
    the CPU for every case here: all are finite with a normal row maximum at both ends.
    One output is not held there: the f32 Hilbert ENVELOPE squares in f32 and states its range, as the f32 mag() does
    (the f64 one is range-safe); test_hilbert_f32_envelope_just_inside_its_range says why and tests it at 2^63 / 2^-62.

(c) Position independence of DCT and Hilbert, whose packed kernels put up to 128 rows into one workgroup: with
    rows_per_wg(N) + 1 rows, a row alone gives the bits it gives in the batch, and a rolled batch the rolled output.
    (The other families have this in their own modules.)

Every case prints `ROWINV` lines with what it measured."""
import math

import numpy as np
import pytest

import sdft_ref as R
import test_gpu_czt as CZT
import test_gpu_dct as DCT
import test_gpu_dft as DFT
import test_gpu_dwt as DWT
import test_gpu_hilbert as HIL
import test_gpu_resample as RES
import test_gpu_stft_pair as STFT
from test_czt_cpu import GRID, grid_direct
from test_czt_cpu import conv_size as czt_conv_size
from test_czt_cpu import row_err as czt_row_err
from test_dct_cpu import NORMS, dct_ref, idct_ref
from test_dft_cpu import conv_size as dft_conv_size
from test_dft_cpu import row_err as dft_row_err
from test_dwt_cpu import wavedec_ref, waverec_ref
from test_gpu_dwt_paths import tile as dwt_tile
from test_gpu_resample_paths import tile_of as upfirdn_tile
from test_hilbert_cpu import MODES, hilbert_ref

pytestmark = pytest.mark.gpu

DTS = ["f32", "f64"]
NPDT = {"f32": np.float32, "f64": np.float64}
EMAX = {"f32": 127, "f64": 1023}
EMIN = {"f32": -126, "f64": -1022}
PREC = {"f32": 24, "f64": 53}
KS = (-20, 17)
ROWS = 4
NS = DCT.NS  # 64 ... 16384
EDGE_NS = [64, 1024, 16384]
EDGES = ["hi", "lo"]


def lg(s):
    return math.ceil(math.log2(s))


def edge_k(dt, s, edge, transforms=1):
    if edge == "hi":
        return EMAX[dt] - transforms * lg(s) - 4
    return EMIN[dt] + PREC[dt] + 2 * lg(s) + 4


def tdt(dt):
    import torch
    return torch.float32 if dt == "f32" else torch.float64


def dev(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(tdt(dt)).cuda()


def gauss(seed, shape, dt):
    """Gaussian values rounded to the dtype, as f64."""
    return np.random.default_rng(seed).standard_normal(shape).astype(NPDT[dt]).astype(np.float64)


def scaling_rows(seed, n, dt):
    """ROWS rows of n: Gaussian, then one impulse and one constant row."""
    x = gauss(seed, (ROWS, n), dt)
    x[ROWS - 2] = 0.0
    x[ROWS - 2, n // 3] = 1.0
    x[ROWS - 1] = 0.75
    return x


def host(out):
    """A tensor or a tuple of tensors -> a list of real numpy arrays in the output's dtype (complex: re, im last)."""
    import torch
    outs = out if isinstance(out, (tuple, list)) else [out]
    torch.cuda.synchronize()
    return [(torch.view_as_real(o) if o.is_complex() else o).cpu().numpy() for o in outs]


def raw(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(a, b):
    return all(x.shape == y.shape and np.array_equal(raw(x), raw(y)) for x, y in zip(host(a), host(b)))


def scales_exactly(out_k, out_1, k):
    """out_k == 2^k out_1 on the raw bits."""
    return all(x.dtype == y.dtype and np.array_equal(raw(x), raw(np.ldexp(y, k))) for x, y in zip(host(out_k), host(out_1)))


def finite(out):
    return all(np.isfinite(a).all() for a in host(out))


def unscaled(out, k):
    """The outputs as f64 times 2^-k (exact)."""
    return [np.ldexp(a.astype(np.float64), -k) for a in host(out)]


def cplx(pair):
    return pair[0] + 1j * pair[1]


def report(family, dt, what, edge, k, share):
    print(f"ROWINV {family} {dt} {what} edge={edge} k={k} share={share:.3f}")


# ---- DCT ------------------------------------------------------------------------------------------------------------

DCT_MODES = [(t, norm, inv) for t in (2, 3) for norm in (None, "ortho") for inv in (False, True)]


def dct_reference(x, t, norm, inv):
    return (idct_ref if inv else dct_ref)(x, t, norm or "backward")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", NS)
def test_dct_scales_exactly(n, dt):
    p = HIL.plan(None, n, dt)
    x = scaling_rows(n, n, dt)
    for t, norm, inv in DCT_MODES:
        base = DCT.run(p, dev(x, dt), t, norm, inv)
        for k in KS:
            assert scales_exactly(DCT.run(p, dev(np.ldexp(x, k), dt), t, norm, inv), base, k), (n, dt, t, norm, inv, k)


def dct_edge_case(n, dt, edge):
    k = edge_k(dt, n, edge)
    xs = np.ldexp(gauss(n + (dt == "f64"), (ROWS, n), dt), k)
    return k, xs, {m: dct_reference(xs, *m) for m in DCT_MODES}


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", EDGE_NS)
def test_dct_range_edges(n, dt, edge):
    p = HIL.plan(None, n, dt)
    k, xs, refs = dct_edge_case(n, dt, edge)
    worst = 0.0
    for (t, norm, inv), want in refs.items():
        y = DCT.run(p, dev(xs, dt), t, norm, inv)
        assert finite(y), (n, dt, edge, t, norm, inv)
        e = DCT.rel_rows(unscaled(y, k)[0], np.ldexp(want, -k))
        b = DCT.TOL[dt] * lg(n)
        worst = max(worst, e / b)
        assert e <= b, (n, dt, edge, t, norm, inv, e)
    report("dct", dt, f"n={n}", edge, k, worst)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [64, 512, 4096, 16384])
def test_dct_rows_do_not_depend_on_their_position(n, dt):
    p = HIL.plan(None, n, dt)
    batch = DCT.rows_per_wg(n) + 1
    x = dev(gauss(3 * n, (batch, n), dt), dt)
    for t in (2, 3):
        for norm in NORMS:
            for inv in (False, True):
                base = DCT.run(p, x, t, norm, inv)
                for b in sorted({0, 1, batch // 2, batch - 1}):
                    assert same_bits(DCT.run(p, x[b:b + 1].clone(), t, norm, inv), base[b:b + 1]), (n, dt, t, norm, inv, b)
                assert same_bits(DCT.run(p, x.roll(1, 0), t, norm, inv), base.roll(1, 0)), (n, dt, t, norm, inv)


# ---- Hilbert --------------------------------------------------------------------------------------------------------

def hilbert_layouts(p, x, dt):
    """The FAST layout and one general one (an odd row stride), asserted to be what they are called."""
    n = x.shape[1]
    xd = dev(x, dt)
    _, xs = HIL.strided(x.shape[0], n, n + 1, dt)
    xs.copy_(xd)
    return (("fast", xd, True), ("stride", xs, False))


def hilbert_run(p, xin, mode, fast):
    y = HIL.run(p, xin, mode)
    assert HIL._fast(p, xin, y, mode) == fast
    return y


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", NS)
def test_hilbert_scales_exactly(n, dt):
    p = HIL.plan(None, n, dt)
    x = scaling_rows(2 * n, n, dt)
    base = {(name, mode): hilbert_run(p, xin, mode, fast) for name, xin, fast in hilbert_layouts(p, x, dt)
            for mode in MODES if mode != "phase"}
    for k in KS:
        xk = np.ldexp(x, k)
        a_ref = hilbert_ref(xk)
        for name, xin, fast in hilbert_layouts(p, xk, dt):
            for mode in MODES:
                y = hilbert_run(p, xin, mode, fast)
                if mode == "phase":  # scale-invariant, and atan2's bits are the math library's: the bound, not the bits
                    e = HIL.err_rows(host(y)[0], a_ref, mode)
                    assert e <= HIL.bound(dt, n, mode), (n, dt, name, k, e)
                elif mode == "envelope" and dt == "f32":
                    # The f32 envelope squares in f32 and promises samples with |a| >= 1.1e-19 only (envelope_of).  At
                    # k = -20 the impulse row has samples below that: x = 0 and Hx a rounding residue of the
                    # butterflies (its true value is 0 at even distances from the impulse), whose square is an f32
                    # subnormal and is rounded absolutely, so sqrt(h h) does not commute with 2^k there (N = 64, 128,
                    # 256 on the device; f64's scaled form has none).  Bits where the scaled sample is inside the
                    # range with a binade to spare; the family's bound everywhere.
                    got, want = host(y)[0], np.ldexp(host(base[name, mode])[0], k)
                    inside = (want >= 2.0 ** -62) | (want == 0)
                    assert inside.mean() > 0.85 and np.array_equal(raw(got)[inside], raw(want)[inside]), (n, name, k)
                    e = HIL.err_rows(np.ldexp(got.astype(np.float64), -k), hilbert_ref(x), mode)
                    assert e <= HIL.bound(dt, n, mode), (n, dt, name, k, e)
                else:
                    assert scales_exactly(y, base[name, mode], k), (n, dt, name, mode, k)


def hilbert_edge_case(n, dt, edge):
    k = edge_k(dt, n, edge)
    xs = np.ldexp(gauss(n + (dt == "f64"), (ROWS, n), dt), k)
    return k, xs, hilbert_ref(xs)


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", EDGE_NS)
def test_hilbert_range_edges(n, dt, edge):
    p = HIL.plan(None, n, dt)
    k, xs, a_ref = hilbert_edge_case(n, dt, edge)
    a_unit = np.ldexp(a_ref.real, -k) + 1j * np.ldexp(a_ref.imag, -k)
    for name, xin, fast in hilbert_layouts(p, xs, dt):
        for mode in MODES:
            if mode == "envelope" and dt == "f32":
                continue  # squares in f32, a stated range: test_hilbert_f32_envelope_just_inside_its_range
            y = hilbert_run(p, xin, mode, fast)
            got = host(y)[0]
            span = (float(np.abs(got).min()), float(np.abs(got).max()))  # a squared envelope: (.., inf) and (0, 0)
            assert np.isfinite(got).all(), (n, dt, edge, name, mode, "not finite", span)
            if mode == "phase":
                got = got.astype(np.float64)
            else:
                got = np.ldexp(got.astype(np.float64), -k)
                if mode == "analytic":
                    got = got[..., 0] + 1j * got[..., 1]
            e = HIL.err_rows(got, a_unit, mode)
            b = HIL.bound(dt, n, mode)
            report("hilbert", dt, f"n={n} {mode} {name}", edge, k, e / b)
            assert e <= b, (n, dt, edge, name, mode, e, span)


def envelope_f32_case(n, k):
    """The tones of test_gpu_hilbert.test_exact_cases (exact bins: |a| = 1 at every sample) times 2^k."""
    nn = np.arange(n)
    ph = np.stack([2 * np.pi * ((b * nn) % n) / n for b in (1, 5, n // 4, n // 2 - 1)])
    xs = np.ldexp(np.cos(ph).astype(np.float32).astype(np.float64), k)
    return xs, hilbert_ref(xs)


@pytest.mark.parametrize("k", [63, -62])
@pytest.mark.parametrize("n", EDGE_NS)
def test_hilbert_f32_envelope_just_inside_its_range(n, k):
    """The f32 ENVELOPE squares in f32 (pdsp_hilbert_kernel.h, envelope_of: the range-safe form cost 6 - 8 % of its
    rate), so it is not held at k_hi / k_lo, where x^2 + Hx^2 is Inf or 0, but just inside its stated range
    1.1e-19 <= |a| <= 1.8e19, at |a| = 2^63 and 2^-62.  The range is per sample (a sample of a Gaussian row far below
    the row's maximum has subnormal squares of its own), so the rows are tones on exact bins, |a| the same at every
    sample; reference, metric and bound are the Hilbert tests' own."""
    p = HIL.plan(None, n, "f32")
    xs, a_ref = envelope_f32_case(n, k)
    a_unit = np.ldexp(a_ref.real, -k) + 1j * np.ldexp(a_ref.imag, -k)
    assert np.abs(np.abs(a_unit) - 1).max() <= 2.0 ** -23 * lg(n)
    for name, xin, fast in hilbert_layouts(p, xs, "f32"):
        got = host(hilbert_run(p, xin, "envelope", fast))[0]
        assert np.isfinite(got).all() and (got >= np.finfo(np.float32).tiny).all(), (n, k, name)
        e = HIL.err_rows(np.ldexp(got.astype(np.float64), -k), a_unit, "envelope")
        b = HIL.bound("f32", n, "envelope")
        report("hilbert", "f32", f"n={n} envelope {name} tones", "hi" if k > 0 else "lo", k, e / b)
        assert e <= b, (n, k, name, e)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", [64, 512, 4096, 16384])
def test_hilbert_rows_do_not_depend_on_their_position(n, dt):
    p = HIL.plan(None, n, dt)
    batch = HIL.rows_per_wg(n) + 1
    x = dev(gauss(5 * n, (batch, n), dt), dt)
    for mode in MODES:
        base = HIL.run(p, x, mode)
        for b in sorted({0, 1, batch // 2, batch - 1}):
            assert same_bits(HIL.run(p, x[b:b + 1].clone(), mode), base[b:b + 1]), (n, dt, mode, b)
        assert same_bits(HIL.run(p, x.roll(1, 0), mode), base.roll(1, 0)), (n, dt, mode)


# ---- STFT / ISTFT: hann, hop N / 4, four frames ---------------------------------------------------------------------

def stft_signals(n, dt):
    """Three signals of four frames: Gaussian, one impulse, a constant."""
    t = n + 3 * (n // 4)
    imp = np.zeros(t)
    imp[n // 3] = 1.0
    return [gauss(n, t, dt), imp, np.full(t, 0.75)]


def istft_spectra(n, dt):
    """(re, im) [4, N / 2 + 1]: Gaussian, one bin of one frame, a constant."""
    bins = n // 2 + 1
    g = gauss(n + 1, (2, ROWS, bins), dt)
    imp = np.zeros((2, ROWS, bins))
    imp[0, 1, bins // 3] = 1.0
    imp[1, 1, bins // 3] = -0.5
    return [g, imp, np.full((2, ROWS, bins), 0.75)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", EDGE_NS)
def test_stft_pair_scales_exactly(n, dt):
    p = HIL.plan(None, n, dt)
    hop = n // 4
    for i, x in enumerate(stft_signals(n, dt)):
        base = p.stft_complex(dev(x, dt), hop, "hann")
        assert base[0].shape == (ROWS, n // 2 + 1)
        for k in KS:
            assert scales_exactly(p.stft_complex(dev(np.ldexp(x, k), dt), hop, "hann"), base, k), ("stft", n, dt, i, k)
    for i, z in enumerate(istft_spectra(n, dt)):
        base = p.istft(dev(z[0], dt), dev(z[1], dt), hop, "hann")
        for k in KS:
            zk = np.ldexp(z, k)
            assert scales_exactly(p.istft(dev(zk[0], dt), dev(zk[1], dt), hop, "hann"), base, k), ("istft", n, dt, i, k)


def stft_edge_case(n, dt, edge, w):
    k = edge_k(dt, n, edge)
    hop = n // 4
    x = np.ldexp(stft_signals(n, dt)[0], k)
    z = np.ldexp(istft_spectra(n, dt)[0], k)
    return k, x, STFT.ref_stft(x, n, hop, w), z, STFT.ref_istft(cplx(z), n, hop, w)


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", EDGE_NS)
def test_stft_pair_range_edges(n, dt, edge):
    p = HIL.plan(None, n, dt)
    hop = n // 4
    k, x, want, z, (iwant, den, ymax) = stft_edge_case(n, dt, edge, STFT.win64(p, "hann"))
    out = p.stft_complex(dev(x, dt), hop, "hann")
    assert finite(out), (n, dt, edge, "stft")
    got = cplx(unscaled(out, k))
    want = np.ldexp(want.real, -k) + 1j * np.ldexp(want.imag, -k)
    e = np.abs(got - want).max() / np.abs(want).max()  # the metric of test_forward_matches_rfft_of_windowed_frames
    b = STFT.FWD_TOL[tdt(dt)] * math.log2(n)
    report("stft", dt, f"n={n}", edge, k, e / b)
    assert e <= b, (n, dt, edge, e)
    out = p.istft(dev(z[0], dt), dev(z[1], dt), hop, "hann")
    assert finite(out), (n, dt, edge, "istft")
    got = unscaled(out, k)[0]
    iwant, ymax = np.ldexp(iwant, -k), math.ldexp(ymax, -k)
    assert got.shape == iwant.shape
    # the metric of test_inverse_matches_the_definition
    zero = (den <= STFT.THR) & (np.abs(den - STFT.THR) > 1e-4 * STFT.THR)
    assert np.all(got[zero] == 0.0)
    good = den >= 1e-3 * den.max()
    e = (np.abs(got - iwant)[good] * np.sqrt(den[good])).max() / (ymax * math.sqrt(math.ceil(n / hop)))
    b = STFT.INV_TOL[tdt(dt)] * math.log2(n)
    report("istft", dt, f"n={n}", edge, k, e / b)
    assert e <= b, (n, dt, edge, e)


# ---- the any-length DFT and the chirp-z transform -------------------------------------------------------------------

def complex_rows(seed, ln, dt, plain=False):
    """(re, im) [2, ROWS, ln]: Gaussian; for the scaling tests one impulse and one constant row among them."""
    z = gauss(seed, (2, ROWS, ln), dt)
    if not plain:
        z[:, ROWS - 2] = 0.0
        z[0, ROWS - 2, ln // 3] = 1.0
        z[1, ROWS - 2, ln // 3] = -0.5
        z[0, ROWS - 1] = 0.75
        z[1, ROWS - 1] = -0.25
    return z


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ln", [3, 97, 1000, 4096])
def test_dft_scales_exactly(ln, dt):
    d = DFT.dft_of(ln)
    z = complex_rows(ln, ln, dt)
    for run in (d.forward, d.inverse):
        base = run(dev(z[0], dt), dev(z[1], dt))
        for k in KS:
            zk = np.ldexp(z, k)
            assert scales_exactly(run(dev(zk[0], dt), dev(zk[1], dt)), base, k), (ln, dt, run.__name__, k)


DFT_EDGE_LS = [32, 512, 4096]  # M = 64, 1024, 8192 (the largest)


def dft_edge_case(ln, dt, edge):
    k = edge_k(dt, dft_conv_size(ln), edge, transforms=2)
    z = np.ldexp(complex_rows(ln + (dt == "f64"), ln, dt, plain=True), k)
    return k, z, np.fft.fft(cplx(z)), np.fft.ifft(cplx(z))


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("ln", DFT_EDGE_LS)
def test_dft_range_edges(ln, dt, edge):
    d = DFT.dft_of(ln)
    assert d.conv_size == 2 * ln
    k, z, fwd, inv = dft_edge_case(ln, dt, edge)
    for name, run, want in (("fwd", d.forward, fwd), ("inv", d.inverse, inv)):
        out = run(dev(z[0], dt), dev(z[1], dt))
        assert finite(out), (ln, dt, edge, name)
        want = np.ldexp(want.real, -k) + 1j * np.ldexp(want.imag, -k)
        e = dft_row_err(cplx(unscaled(out, k)), want)
        b = DFT.bound(dt, ln)
        report("dft", dt, f"L={ln} M={d.conv_size} {name}", edge, k, e / b)
        assert e <= b, (ln, dt, edge, name, e)


CZT_SHAPES = CZT.BITS
RADII = [1.0, 0.999]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("ln,bins", CZT_SHAPES)
def test_czt_scales_exactly(ln, bins, radius, dt):
    c = CZT.czt_of(ln, bins, CZT.P / GRID, CZT.Q / GRID, radius)
    z = complex_rows(ln + bins, ln, dt)
    base = c.forward(dev(z[0], dt), dev(z[1], dt))
    for k in KS:
        zk = np.ldexp(z, k)
        assert scales_exactly(c.forward(dev(zk[0], dt), dev(zk[1], dt)), base, k), (ln, bins, radius, dt, k)


def czt_edge_case(ln, bins, radius, dt, edge, p, q):
    k = edge_k(dt, czt_conv_size(ln, bins), edge, transforms=2)
    z = np.ldexp(complex_rows(1000 * ln + 2 * bins + (dt == "f64"), ln, dt, plain=True), k)
    return k, z, grid_direct(cplx(z), bins, p, q, radius, extended=(dt == "f64"))


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("ln,bins", CZT_SHAPES)
def test_czt_range_edges(ln, bins, radius, dt, edge):
    c = CZT.czt_of(ln, bins, CZT.P / GRID, CZT.Q / GRID, radius)
    k, z, want = czt_edge_case(ln, bins, radius, dt, edge, CZT.P, CZT.Q)
    out = c.forward(dev(z[0], dt), dev(z[1], dt))
    assert finite(out), (ln, bins, radius, dt, edge)
    want = np.ldexp(want.real, -k) + 1j * np.ldexp(want.imag, -k)
    e = czt_row_err(cplx(unscaled(out, k)), want, cplx(np.ldexp(z, -k)), radius)
    b = CZT.bound(dt, ln, bins)
    report("czt", dt, f"L={ln} K={bins} M={c.conv_size} radius={radius}", edge, k, e / b)
    assert e <= b, (ln, bins, radius, dt, edge, e)


# ---- DWT ------------------------------------------------------------------------------------------------------------

def dwt_tiled(dt):
    return (12288 if dt == "f32" else 6144, 4, "db4")  # the rule tiles these (tests/test_gpu_dwt_paths.py)


DWT_RESIDENT = [(96, 3, "db2"), (96, 3, "f32"), (1024, 6, "db4")]


def dwt_handle(key, levels, dt):
    import pragma_dsp_amd as pd
    return pd.Dwt(DWT.wavelet(key), levels, "cuda:0", tdt(dt))


def dwt_is_resident(w, levels, n, dt):
    return [dwt_tile(w.ntaps, levels, n, tdt(dt), inv)["resident"] for inv in (False, True)]


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", DWT_RESIDENT + ["tiled"], ids=lambda c: c if isinstance(c, str) else f"{c[0]}-{c[1]}-{c[2]}")
def test_dwt_scales_exactly(case, dt):
    n, levels, key = dwt_tiled(dt) if case == "tiled" else case
    w = dwt_handle(key, levels, dt)
    assert dwt_is_resident(w, levels, n, dt) == ([0, 0] if case == "tiled" else [1, 1])
    x = scaling_rows(n + levels, n, dt)
    for run in (w.forward, w.inverse):
        base = run(dev(x, dt))
        for k in KS:
            assert scales_exactly(run(dev(np.ldexp(x, k), dt)), base, k), (n, levels, key, dt, run.__name__, k)


DWT_EDGE = [(96, 3, "db2"), (96, 3, "f32"), (1024, 6, "db4"), (16384, 4, "db4")]


def dwt_edge_case(n, levels, key, dt, edge):
    k = edge_k(dt, n, edge)
    cs = DWT.case(n, levels, key, tdt(dt), ROWS)
    xs, c = np.ldexp(cs["x"], k), np.ldexp(cs["c"], k)
    return k, cs, xs, c, wavedec_ref(xs, cs["h"], levels), waverec_ref(c, cs["h"], levels)


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n,levels,key", DWT_EDGE, ids=[f"{n}-{j}-{key}" for n, j, key in DWT_EDGE])
def test_dwt_range_edges(n, levels, key, dt, edge):
    w = dwt_handle(key, levels, dt)
    k, cs, xs, c, fwd, inv = dwt_edge_case(n, levels, key, dt, edge)
    # the bounds of case() are sums of absolute terms of the unit rows: they hold got 2^-k against ref 2^-k
    for name, run, src, want, bound in (("forward", w.forward, xs, fwd, cs["fwd_bound"]),
                                        ("inverse", w.inverse, c, inv, cs["inv_bound"])):
        out = run(dev(src, dt))
        assert finite(out), (n, levels, key, dt, edge, name)
        DWT.hold(unscaled(out, k)[0], np.ldexp(want, -k), bound, f"ROWINV dwt {dt} {key} n={n} J={levels} {name} edge={edge} k={k}")


# ---- polyphase resampling -------------------------------------------------------------------------------------------

RATIOS = [(3, 2), (1, 4), (7, 1)]
TILED_LEN = 20011


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("up,down", RATIOS)
def test_upfirdn_scales_exactly(up, down, dt):
    import pragma_dsp_amd as pd
    r = pd.Resampler(up, down, device="cuda:0", dtype=tdt(dt))
    assert upfirdn_tile(r.up, r.down, r.ntaps, r.output_len(TILED_LEN), tdt(dt)).tiles >= 3
    x = scaling_rows(up + down, TILED_LEN, dt)
    base = r.apply(dev(x, dt))
    for k in KS:
        assert scales_exactly(r.apply(dev(np.ldexp(x, k), dt)), base, k), (up, down, dt, k)


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("n", EDGE_NS)
@pytest.mark.parametrize("up,down", RATIOS)
def test_upfirdn_range_edges(up, down, n, dt, edge):
    import pragma_dsp_amd as pd
    r = pd.Resampler(up, down, device="cuda:0", dtype=tdt(dt))
    k = edge_k(dt, n, edge)
    xs = np.ldexp(RES.signal((ROWS, n), tdt(dt), n + up), k)
    # check() computes the reference and the bound (T + 2) eps sum |h| |x| from the scaled rows themselves; neither squares
    y = RES.check(r, xs, tdt(dt), f"ROWINV upfirdn {up}/{down} edge={edge} k={k}")
    assert finite(y), (up, down, n, dt, edge)


# ---- the sliding DFT ------------------------------------------------------------------------------------------------

SDFT_WINDOWS = ["rect", "hann"]


def sdft_run(n, bins, hop, win, x, dt):
    import pragma_dsp_amd as pd
    return pd.SlidingDft(n, bins, hop=hop, window=win).forward(dev(x, dt))


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("win", SDFT_WINDOWS)
@pytest.mark.parametrize("n", R.SIZES[:2] + (64,))  # the two smallest sizes, and the smallest that has every window
def test_sdft_scales_exactly(n, win, dt):
    t = 3 * n + 7
    x = scaling_rows(n, t, dt)
    # One legitimate exception, N = 2 in f32, the constant row, found on the device and reproduced bit for bit by
    # sdft_ref.emulate(exact=True): at the odd bins tab[1] = e^(-i pi b) and tab[N] = e^(-2 i pi b) have imaginary
    # parts of about 2^-64, the sines of multiples of a long double pi.  The row's leading terms x0 - x1 cancel
    # exactly, and what is left of the real part is x times the product of two such residues (the fma of sdft_cmul's
    # real part in v = S + tab[N] Pex): 1.9e-39 at unit scale, an f32 subnormal, whose rounding is absolute, so it does
    # not commute with 2^k.  The premise "away from the subnormals" fails, not the kernel's linearity; that row is held
    # to the family's bound instead, the other rows to their bits.
    exact = ROWS - 1 if (n, dt) == (2, "f32") else ROWS
    for hop in (1, n + 1):  # n + 1: every frame starts in another chunk
        base = sdft_run(n, R.bins_of(n), hop, win, x, dt)
        assert base[0].shape == (ROWS, len(R.bins_of(n)), R.frames_of(n, hop, t))
        for k in KS:
            out = sdft_run(n, R.bins_of(n), hop, win, np.ldexp(x, k), dt)
            assert scales_exactly([o[:exact] for o in out], [o[:exact] for o in base], k), (n, win, dt, hop, k)
            if exact < ROWS:
                re, im = R.direct(x[exact:], n, R.bins_of(n), hop, win)
                e = R.err_units(cplx(unscaled(out, k))[exact:], re, im, n, dt, np.abs(x[exact:]).max())
                assert e <= R.BOUND[dt], (n, win, dt, hop, k, e)


def sdft_edge_case(n, win, hop, dt, edge):
    t = 2 * n + 1
    k = edge_k(dt, t, edge)
    x = gauss([n, t], (ROWS, t), "f32")  # exact in f32, as sdft_ref.signal
    fr = R.pick_frames(n, hop, t)
    xs = np.ldexp(x, k)
    re, im = R.direct(xs, n, R.bins_of(n), hop, win, fr)
    return k, x, xs, fr, re, im


@pytest.mark.parametrize("edge", EDGES)
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("win", SDFT_WINDOWS)
@pytest.mark.parametrize("n", EDGE_NS)
def test_sdft_range_edges(n, win, dt, edge):
    worst = 0.0
    for hop in (1, n + 1):
        k, x, xs, fr, re, im = sdft_edge_case(n, win, hop, dt, edge)
        out = sdft_run(n, R.bins_of(n), hop, win, xs, dt)
        assert finite(out), (n, win, dt, edge, hop)
        got = cplx(unscaled(out, k))[:, :, fr]
        e = R.err_units(got, np.ldexp(re, -k), np.ldexp(im, -k), n, dt, np.abs(x).max())
        worst = max(worst, e / R.BOUND[dt])
        assert e <= R.BOUND[dt], (n, win, dt, edge, hop, e)
    report("sdft", dt, f"N={n} {win}", edge, k, worst)

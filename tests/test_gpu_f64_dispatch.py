"""The f64 device family against the f64 oracle, path by path.  The dispatcher picks among a dozen f64 kernel
forms by size, batch, the 8- / 16- / 32-byte alignment of each plane (offsets of 1, 2 and 4 doubles), frame
length, stride, window, sides and requested outputs (pdsp_dispatch.inc: run_complex, spectrum_impl).  Each case
below names the kernel it is meant to reach; the seeded fuzzes cover the combinations in between.

Bounds (include/pdsp_hip.h: ~1e-15 relative to max): transforms 1e-14 up to N = 2^13 and 1e-13 above, amplitudes
1e-13, phase 1e-9 rad where the amplitude is above 1e-6 of its row's maximum, peak the oracle's bin, its two-sided
mirror or a bin whose amplitude ties within 1e-13 of the maximum.  An f32-rounded table or window is ~1e5 above
them.  The worst error of each case is recorded as a junit property (`worst_*`)."""
import zlib

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

AMP_TOL = 1e-13
PHASE_TOL = 1e-9
WINDOWS = ("rect", "hann", "hamming", "blackman")


def _tf_tol(n):
    return 1e-14 if n <= 1 << 13 else 1e-13


def _view(torch, rows, length, off, stride=None):
    """[rows, length] float64 view whose first element is `off` doubles past a 512-byte aligned base (offsets 1, 2, 4
    give 8-, 16- and 32-byte alignment), rows `stride` apart; the storage covers every element read."""
    stride = length if stride is None else stride
    flat = torch.zeros(max(rows - 1, 0) * stride + length + off + 8, dtype=torch.float64, device="cuda")
    return torch.as_strided(flat, (rows, length), (stride, 1), off)


def _plan(plans, n):
    import torch
    from pragma_dsp_amd.batch import BatchedFft
    if n not in plans:
        plans[n] = BatchedFft(n, "cuda:0", dtype=torch.float64)
    return plans[n]


def _run_transform(plan, kind, re, im, offs, out_mode="disjoint"):
    """One transform call with its planes at `offs` (doubles past an aligned base; re_in, im_in, re_out, im_out).
    out_mode: "disjoint"; "inplace" (out planes are the input planes); "overlap" (out.real starts inside the
    input's real buffer, so planes_overlap() is true without equal pointers).  Returns (got, want) complex."""
    import torch
    batch, n = re.shape
    dre = _view(torch, batch, n, offs[0])
    dre.copy_(torch.from_numpy(re))
    dim = None
    if kind != "real":
        dim = _view(torch, batch, n, offs[1])
        dim.copy_(torch.from_numpy(im))
    if out_mode == "inplace":
        out = (dre, dim if dim is not None else _view(torch, batch, n, offs[3]))
    elif out_mode == "overlap":
        # one buffer holds the real input and, shifted by half a plane plus offs[2] doubles, the real output
        shift = (batch * n) // 2 + offs[2]
        flat = torch.zeros(batch * n + shift + 8, dtype=torch.float64, device="cuda")
        src = torch.as_strided(flat, (batch, n), (n, 1), 0)
        src.copy_(dre)
        dre = src
        out = (torch.as_strided(flat, (batch, n), (n, 1), shift), _view(torch, batch, n, offs[3]))
    else:
        out = (_view(torch, batch, n, offs[2]), _view(torch, batch, n, offs[3]))
    o = _oracle_plan(n)
    if kind == "complex":
        gre, gim = plan.forward(dre, dim, out=out)
        wre, wim = o.forward_complex(re, im)
    elif kind == "real":
        gre, gim = plan.forward(dre, out=out)
        wre, wim = o.forward(re)
    else:
        gre, gim = plan.inverse(dre, dim, out=out)
        wre, wim = o.inverse(re, im)
    assert gre is out[0] and gim is out[1]
    return gre.cpu().numpy() + 1j * gim.cpu().numpy(), wre + 1j * wim


_ORACLE = {}


def _oracle_plan(n):
    import oracle
    if n not in _ORACLE:
        oracle.build()
        _ORACLE[n] = oracle.Plan(n)
    return _ORACLE[n]


# ---- a. deterministic path table: transforms --------------------------------------------------------------------
# (id naming the intended kernel, log2 sizes, batch, kinds, plane offsets re_in / im_in / re_out / im_out, out mode)
TRANSFORM_PATHS = [
    ("fft_tiny_staged_kernel-aligned32", range(1, 5), 37, ("complex", "real", "inverse"), (0, 4, 4, 0), "disjoint"),
    ("fft_stockham_kernel-tiny-re_in16", range(1, 5), 37, ("complex", "real", "inverse"), (2, 0, 0, 0), "disjoint"),
    ("fft_stockham_kernel-tiny-im_out8", range(1, 5), 5, ("complex", "real", "inverse"), (0, 0, 0, 1), "disjoint"),
    ("fft_stockham_kernel-n1", range(0, 1), 9, ("complex", "real", "inverse"), (1, 3, 2, 0), "disjoint"),
    ("fft_staged_kernel-aligned32", range(5, 8), 33, ("complex", "real", "inverse"), (4, 0, 0, 4), "disjoint"),
    ("fft_stockham_kernel-staged-im_in16", range(5, 8), 33, ("complex", "inverse"), (0, 2, 0, 0), "disjoint"),
    ("fft_stockham_kernel-staged-re_out8", range(5, 8), 7, ("complex", "real", "inverse"), (0, 0, 3, 0), "disjoint"),
    ("fft_stockham_kernel-256-aligned32", range(8, 9), 5, ("complex", "real", "inverse"), (0, 0, 0, 0), "disjoint"),
    ("fft_split2_kernel-in16", range(13, 14), 3, ("complex", "inverse"), (2, 2, 1, 3), "disjoint"),
    ("fft_stockham_kernel-8192-re_in8", range(13, 14), 3, ("complex", "inverse"), (1, 0, 0, 0), "disjoint"),
    ("fft_stockham_kernel-8192-im_in8", range(13, 14), 2, ("complex", "inverse"), (0, 3, 0, 0), "disjoint"),
    ("fft_real_kernel-8192-re_in16", range(13, 14), 3, ("real",), (2, 0, 1, 3), "disjoint"),
    ("fft_stockham_kernel-8192-real-re_in8", range(13, 14), 3, ("real",), (1, 0, 0, 0), "disjoint"),
    ("fft_real_kernel-16384-batch8", range(14, 15), 8, ("real",), (0, 0, 3, 1), "disjoint"),
    ("fourstep-16384-real-batch7", range(14, 15), 7, ("real",), (0, 0, 0, 0), "disjoint"),
    ("fourstep-16384-real-batch8-re_in8", range(14, 15), 8, ("real",), (1, 0, 0, 0), "disjoint"),
    ("fourstep_cols_kernel-misaligned-batch1", range(14, 18), 1, ("complex", "real", "inverse"), (1, 3, 1, 3), "disjoint"),
    ("fourstep_cols_kernel-misaligned-batch3", range(14, 18), 3, ("complex", "real", "inverse"), (3, 1, 2, 1), "disjoint"),
    ("bigfft_transpose_kernel-disjoint", range(18, 21), 1, ("complex", "real", "inverse"), (0, 1, 2, 3), "disjoint"),
    ("bigfft_transpose_kernel-inplace", range(18, 21), 2, ("complex", "real", "inverse"), (0, 0, 0, 4), "inplace"),
    ("bigfft_transpose_kernel-overlap", range(18, 20), 2, ("complex", "real", "inverse"), (0, 4, 1, 0), "overlap"),
]


@pytest.mark.parametrize("path", TRANSFORM_PATHS, ids=[p[0] for p in TRANSFORM_PATHS])
def test_transform_paths(record_property, path):
    name, sizes, batch, kinds, offs, mode = path
    rng = np.random.default_rng(_seed(name))
    plans, worst = {}, 0.0
    for log2n in sizes:
        n = 1 << log2n
        for kind in kinds:
            re, im = rng.standard_normal((batch, n)), rng.standard_normal((batch, n))
            got, want = _run_transform(_plan(plans, n), kind, re, im, offs, mode)
            err = rel_err(got, want)
            worst = max(worst, err)
            assert err <= _tf_tol(n), (name, log2n, batch, kind, offs, mode, err)
    record_property("worst_rel_err", worst)


@pytest.mark.parametrize("inverse", [False, True])
def test_interleaved_single_pass(oracle_mod, record_property, inverse):
    """forward_interleaved / inverse_interleaved (LoadInterleaved / StoreInterleaved on fft_stockham_kernel) at every
    single-pass f64 size, ragged batches."""
    import torch
    rng = np.random.default_rng(7 + inverse)
    plans, worst = {}, 0.0
    for log2n in range(0, 14):
        n = 1 << log2n
        batch = int(rng.integers(1, 40)) | 1
        re, im = rng.standard_normal((batch, n)), rng.standard_normal((batch, n))
        z = torch.from_numpy(re + 1j * im).cuda()
        plan = _plan(plans, n)
        got = (plan.inverse_interleaved(z) if inverse else plan.forward_interleaved(z)).cpu().numpy()
        wre, wim = (oracle_mod.Plan(n).inverse(re, im) if inverse else oracle_mod.Plan(n).forward_complex(re, im))
        err = rel_err(got, wre + 1j * wim)
        worst = max(worst, err)
        assert err <= _tf_tol(n), (log2n, batch, inverse, err)
    record_property("worst_rel_err", worst)


# ---- spectrum checks ----------------------------------------------------------------------------------------------

def _seed(name):
    return zlib.crc32(name.encode())


def _window_arg(torch, window, n, win_off):
    """(what BatchedFft.spectrum gets, the f64 table the oracle gets).  "custom": the caller's own table (the same
    for every call of one size), a plain tensor at `win_off` doubles past an aligned base."""
    import oracle
    if window == "custom":
        w = 0.25 + np.random.default_rng(n).random(n)
        dw = _view(torch, 1, n, win_off)[0]
        dw.copy_(torch.from_numpy(w))
        return dw, w
    return window, (oracle.create_window(window, n) if (window != "rect" and n > 1) else None)


def _check_spectrum(plan, x, off, window, sides, want_phase, want_peak, ctx, win_off=0, scale=1.0,
                    stride=None, n_frames=None):
    """One pdsp_spectrum_f64 call on frames x (host [batch, length], or one signal read with row stride `stride`
    for the STFT) at `off` doubles; checks amplitude, phase and peak against the oracle on the materialised
    frames.  Returns (amplitude, phase or None, peak or None as numpy, worst amplitude error, worst phase error)."""
    import torch
    n = plan.size
    xs = x * scale
    if stride is None:
        batch, length = x.shape
        dx = _view(torch, batch, length, off)
        dx.copy_(torch.from_numpy(xs))
        frames = np.zeros((batch, n))
        frames[:, :min(n, length)] = xs[:, :n]
    else:  # STFT: frame b = signal[b * hop : b * hop + N]
        sig = _view(torch, 1, x.size, off)[0]
        sig.copy_(torch.from_numpy(xs))
        batch = n_frames
        frames = np.stack([xs[b * stride:b * stride + n] for b in range(batch)])
    win, wtab = _window_arg(torch, window, n, win_off)
    if stride is None:
        amp, ph, pk = plan.spectrum(dx, win, sides, want_phase=want_phase, want_peak=want_peak)
    else:
        amp, ph, pk = plan.stft(sig, stride, win, sides, want_phase=want_phase, want_peak=want_peak)
    wamp, wph, wpk = _oracle_plan(n).spectrum_batch(frames, window=wtab, two_sided=(sides == "two"),
                                                    want_phase=True, want_peak=True)
    a = amp.cpu().numpy()
    assert a.shape == wamp.shape, ctx
    assert np.isfinite(a).all(), ctx
    aerr = rel_err(a, wamp)
    assert aerr <= AMP_TOL, (ctx, aerr)
    top = wamp.max(axis=-1, keepdims=True)
    perr = 0.0
    ph = ph.cpu().numpy() if ph is not None else None
    pk = pk.cpu().numpy() if pk is not None else None
    if want_phase:
        mask = wamp > 1e-6 * top
        d = np.abs((ph - wph + np.pi) % (2 * np.pi) - np.pi)
        perr = float(d[mask].max(initial=0))
        assert perr <= PHASE_TOL, (ctx, perr)
    else:
        assert ph is None, ctx
    if want_peak:
        p = pk
        for b in range(batch):
            ok = p[b] == wpk[b] or (sides == "two" and p[b] == (n - wpk[b]) % n) or \
                abs(wamp[b, p[b]] - wamp[b, wpk[b]]) <= AMP_TOL * top[b, 0]
            assert ok, (ctx, b, int(p[b]), int(wpk[b]))
    return a, ph, pk, aerr, perr


# (id naming the intended kernel, log2 sizes, batch, [(length delta, frame offset, window, window offset, sides,
#  want_phase, want_peak)]).  Length delta: frames of N + delta samples (the row stride is the frame length).
SPECTRUM_PATHS = [
    ("fft_tiny_staged_kernel-amp", range(1, 6), 9,
     [(0, 0, "rect", 0, "one", False, False), (0, 4, "hamming", 0, "two", False, True),
      (0, 0, "custom", 1, "one", False, True)]),
    ("fft_stockham_kernel-LoadFrameWindowed", range(0, 6), 7,
     [(0, 0, "hamming", 0, "one", True, True), (0, 2, "rect", 0, "one", False, False),
      (0, 1, "rect", 0, "two", False, True), (-1, 0, "rect", 0, "one", False, False),
      (1, 0, "hamming", 0, "two", False, False), (3, 4, "custom", 2, "one", True, False)]),
    ("spectrum_packed_kernel-fast", range(6, 15), 5,
     [(0, 0, "rect", 0, "one", False, False), (0, 2, "hann", 0, "one", False, True),
      (2, 0, "blackman", 0, "one", False, False), (0, 4, "custom", 2, "one", False, True)]),
    ("spectrum_packed_kernel-general", range(6, 15), 5,
     [(0, 1, "hann", 0, "one", False, True), (1, 0, "rect", 0, "one", False, False),
      (-3, 0, "hamming", 0, "one", False, True), (0, 0, "hann", 0, "two", False, True),
      (0, 0, "blackman", 0, "one", True, False), (0, 0, "custom", 1, "one", False, False)]),
    ("fourstep_out_kernel-amp", range(15, 18), 2,
     [(0, 0, "hann", 0, "one", True, True), (-5, 1, "rect", 0, "one", False, True),
      (7, 0, "custom", 3, "one", False, False), (0, 2, "blackman", 0, "two", True, True)]),
    ("bigfft_transpose_kernel-amp", range(18, 19), 2,
     [(0, 0, "hann", 0, "one", True, True), (-5, 1, "rect", 0, "one", False, True),
      (7, 0, "custom", 3, "one", False, False), (0, 2, "blackman", 0, "two", True, True)]),
]
_SPECTRUM_IDS = [p[0] for p in SPECTRUM_PATHS]


def _spectrum_rows(path, rng):
    """Every call of one SPECTRUM_PATHS row: (n, frames, ctx, options)."""
    name, sizes, batch, variants = path
    for log2n in sizes:
        n = 1 << log2n
        for (dl, off, window, win_off, sides, want_phase, want_peak) in variants:
            length = max(1, n + dl)
            if n <= 2 and window in ("hann", "blackman"):
                window = "hamming"  # hann(2) = 0, blackman(2) ~ 1e-17: nothing but rounding left to compare
            x = rng.standard_normal((batch, length))
            ctx = (name, log2n, batch, length, off, window, win_off, sides, want_phase, want_peak)
            yield n, x, ctx, dict(off=off, window=window, win_off=win_off, sides=sides, want_phase=want_phase,
                                  want_peak=want_peak)


@pytest.mark.parametrize("path", SPECTRUM_PATHS, ids=_SPECTRUM_IDS)
def test_spectrum_paths(record_property, path):
    rng = np.random.default_rng(_seed(path[0]))
    plans, worst_a, worst_p = {}, 0.0, 0.0
    for n, x, ctx, o in _spectrum_rows(path, rng):
        *_, aerr, perr = _check_spectrum(_plan(plans, n), x, o["off"], o["window"], o["sides"], o["want_phase"],
                                         o["want_peak"], ctx, win_off=o["win_off"])
        worst_a, worst_p = max(worst_a, aerr), max(worst_p, perr)
    record_property("worst_amp_rel_err", worst_a)
    record_property("worst_phase_rad", worst_p)


# ---- e. the ends of the double range ----------------------------------------------------------------------------

@pytest.mark.parametrize("path", SPECTRUM_PATHS, ids=_SPECTRUM_IDS)
@pytest.mark.parametrize("log2_scale", [980, -980])
def test_spectrum_range_ends(record_property, path, log2_scale):
    """Frames times 2^980 / 2^-980 (exact): |X| must come from hypot -- finite, nonzero, equal to the scaled
    unit-scale amplitude and to the oracle within 1e-13.  sqrt(re^2 + im^2) gives inf / 0 here."""
    scale = 2.0 ** log2_scale
    rng = np.random.default_rng(_seed(path[0]))
    plans, worst = {}, 0.0
    for n, x, ctx, o in _spectrum_rows(path, rng):
        args = (o["off"], o["window"], o["sides"], o["want_phase"], o["want_peak"])
        plan = _plan(plans, n)
        unit, *_ = _check_spectrum(plan, x, *args, ctx, win_off=o["win_off"])
        big, _, _, aerr, _ = _check_spectrum(plan, x, *args, ctx + (log2_scale,), win_off=o["win_off"], scale=scale)
        live = unit > 1e-12 * unit.max(axis=-1, keepdims=True)  # bins whose scaled value is a normal double
        assert np.isfinite(big).all() and (big[live] != 0).all(), (ctx, log2_scale)
        err = rel_err(big / scale, unit)
        worst = max(worst, err, aerr)
        assert err <= AMP_TOL, (ctx, log2_scale, err)
    record_property("worst_amp_rel_err", worst)


# ---- b. seeded transform fuzz ------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(6))
def test_transform_fuzz_f64(record_property, seed):
    rng = np.random.default_rng(5000 + seed)
    plans, worst = {}, 0.0
    for _ in range(40):
        log2n = int(rng.integers(0, 21))
        n = 1 << log2n
        batch = int(rng.integers(1, max(2, min(64, (1 << 21) // n)) + 1))
        offs = tuple(int(v) for v in rng.integers(0, 5, size=4))
        kind = str(rng.choice(["complex", "real", "inverse"]))
        re, im = rng.standard_normal((batch, n)), rng.standard_normal((batch, n))
        got, want = _run_transform(_plan(plans, n), kind, re, im, offs)
        err = rel_err(got, want)
        worst = max(worst, err)
        assert err <= _tf_tol(n), (log2n, batch, offs, kind, err)
        if log2n >= 18:
            plans.pop(n).close()  # the general four-step path's scratch goes back with its plan
    record_property("worst_rel_err", worst)


# ---- c. seeded spectrum fuzz -------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(6))
def test_spectrum_fuzz_f64(record_property, seed):
    rng = np.random.default_rng(6000 + seed)
    plans, worst_a, worst_p = {}, 0.0, 0.0
    for _ in range(30):
        log2n = int(rng.integers(0, 19))
        n = 1 << log2n
        batch = int(rng.integers(2, max(3, min(48, (1 << 20) // n)) + 1))
        k = int(rng.integers(1, 9))
        length = int(rng.choice([n, n, max(1, n - k), n + k]))
        off = int(rng.integers(0, 5))
        window = str(rng.choice(WINDOWS + ("custom",)))
        if n <= 2 and window in ("hann", "blackman"):
            window = "hamming"
        win_off = int(rng.integers(0, 5))
        sides = str(rng.choice(["one", "two"]))
        want_phase, want_peak = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        x = rng.standard_normal((batch, length))
        zero = int(rng.integers(0, batch))
        x[zero] = 0.0  # one all-zero frame per batch: exact zeros, peak 0
        ctx = (log2n, batch, length, off, window, win_off, sides, want_phase, want_peak, zero)
        amp, ph, pk, aerr, perr = _check_spectrum(_plan(plans, n), x, off, window, sides, want_phase, want_peak, ctx,
                                                  win_off)
        assert not amp[zero].any(), ctx
        # a zero bin's phase is atan2 of signed zeros (a window value of -1e-17 makes -0): 0 or +-pi, nothing else
        assert ph is None or np.isin(ph[zero], (0.0, np.pi, -np.pi)).all(), ctx
        assert pk is None or pk[zero] == 0, ctx
        worst_a, worst_p = max(worst_a, aerr), max(worst_p, perr)
        if log2n >= 18:
            plans.pop(n).close()
    record_property("worst_amp_rel_err", worst_a)
    record_property("worst_phase_rad", worst_p)


# ---- d. f64 STFT -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("log2n", [3, 5, 6, 9, 12, 14, 15, 16])
def test_stft_f64(record_property, log2n):
    """plan.stft reads one signal with row stride hop (frame_stride != frame_len): hops 1, odd, N/4 and N."""
    n = 1 << log2n
    rng = np.random.default_rng(700 + log2n)
    plans, worst, worst_p = {}, 0.0, 0.0
    plan = _plan(plans, n)
    for hop, frames, window, sides, want_phase, want_peak in [
            (1, 5, "hann", "one", True, True), ((n // 3) | 1, 4, "rect", "two", False, True),
            (max(1, n // 4), 6, "blackman", "one", False, False), (n, 3, "hamming", "one", True, False)]:
        length = n + (frames - 1) * hop
        x = rng.standard_normal(length)
        ctx = ("stft", log2n, hop, frames, window, sides, want_phase, want_peak)
        for off in (0, 1):
            *_, aerr, perr = _check_spectrum(plan, x, off, window, sides, want_phase, want_peak, ctx + (off,),
                                             stride=hop, n_frames=frames)
            worst, worst_p = max(worst, aerr), max(worst_p, perr)
    record_property("worst_amp_rel_err", worst)
    record_property("worst_phase_rad", worst_p)

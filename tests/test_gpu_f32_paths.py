"""The f32 transform and spectrum kernels path by path, against f64 references of the f32-rounded inputs.

The dispatcher (pdsp_dispatch.inc: pick_transform, pick_spectrum and the launchers that switch on their result) picks
among about twenty f32 kernel forms by size, plane alignment, aliasing, frame length, stride, window identity, sides,
requested outputs and four development switches.  expected_path() below restates those predicates independently.
Before every call the library itself is asked (pdsp_dev_transform_path_f32 / pdsp_dev_spectrum_path_f32, on the
call's own pointers and under its switch values) which path it takes; path_names() puts the answer into
expected_path()'s vocabulary and the two sets must be EQUAL, so a change of the dispatch rule fails here and does not
silently move a case to another kernel.  Every case then asserts the path it names on the library's answer, and
test_path_table_reaches_every_path checks that the tables reach each name in REQUIRED.

References: numpy.fft in f64 on the f32-rounded inputs (its own error, ~1e-16, is negligible).  Spectrum cases apply
the scaling of spectrum(): s_edge = 1/N at bins 0 and N/2 one-sided, s_mid = 2/N elsewhere (1/N everywhere two-sided);
reference_spectrum() is pinned once against the C oracle.  A table window is compared as its f32 table; a plan window
that the kernel evaluates in registers (fused cosine sum) is compared with the f64 window, so the fused form's own
error is part of what is measured.

Metric, per row: max_k |got_k - ref_k| / scale_k, scale_k = max(rms(ref), |ref_k|, max|ref| / 16), where
rms(ref) = ||ref||_2 / sqrt(len) -- for a forward transform ||x||_2 (Parseval).  Unlike max|got - ref| / max|ref|
it does not loosen when the row has a peak: a bin next to a peak is held to rms, or at most to 1/16 of the peak.
The two other terms admit what f32 rounding does by itself: a bin's own error scales with the bin, and the rounding
of a peak's partial sums lands in the bins around it at about one ulp of the peak (measured ~3e-8 max|X| at every N,
which against rms alone would need bounds growing like sqrt(N)).  A fused cosine-sum window is a few f32 ulps off in
absolute terms, so its rows are also scaled by the rms amplitude of the unwindowed frame.  Amplitude rows use the
same metric over the bins returned; phase is checked where |X_k| >= 1e-3 rms, within PHASE_C * bound * scale_k /
|X_k| rad.  Inputs per case: Gaussian rows, an off-bin sinusoid plus 1e-4 noise, an impulse at a random position
(its spectrum is the twiddle sequence itself), a constant and an all-zero row, each scaled by its own power of two.

The error grows with log2 N, so the bounds do too (TOL[kind] x log2 N, log2 N taken as 1 for N = 1).  Each bound is
2.4-2.8x the worst error measured on an MI355X across this file (recorded per case as `worst_*` junit properties, in
units of log2 N; the inputs are seeded, so the measurement repeats bit for bit):
  forward transforms  1.02e-7 x log2 N (fft_staged_kernel; tile passes 8.9e-8), bound 2.5e-7 x log2 N;
  inverse transforms  9.1e-8 x log2 N (fft_staged_kernel), bound 2.5e-7 x log2 N;
  amplitude rows      1.66e-7 x log2 N (spectrum_packed_kernel, blackman table; packed tile chain 1.65e-7),
                      bound 4e-7 x log2 N;
  phase               0.39 of its bound at most.
The old suite's 1e-5 of max|X| is 7-20x above these bounds (in its own units) for a Gaussian row of N <= 16384, and
far more for a row with a peak.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 1024  # floats of NaN before and after every buffer: 4 KiB margins
TOL = {"fwd": 2.5e-7, "inv": 2.5e-7, "amp": 4e-7}  # x log2 N
PHASE_C = 0.5
SENT_I32 = -0x3e5a3e5a  # int32 sentinel of the index and record buffers
SR = 48000.0


def lg(n):
    return max(n.bit_length() - 1, 1)


def bound(kind, n):
    return TOL[kind] * lg(n)


# ---- the dispatch, restated -------------------------------------------------------------------------------------

DEFAULT_SWITCHES = {"split16k": 1, "twopass": 1, "staged_small": 1, "fused_window": 1}


def _a(nbytes, *offs):
    """Are the planes at these float offsets (past a 4 KiB aligned base) multiples of nbytes?  None = no plane."""
    return all(o is None or (4 * o) % nbytes == 0 for o in offs)


def _three(lg_):
    l0 = lg_ // 3
    l1 = (lg_ - l0) // 2
    return [l0, l1, lg_ - l0 - l1]


def _tile_names(ls, first_cols_ok, tp):
    """tile_cols512_kernel / tile_rows512_kernel where a factor is 2^9 (tile_pass), tile_pass_kernel elsewhere."""
    names = set()
    wide = not (tp & 2)
    for i, l in enumerate(ls):
        last = i == len(ls) - 1
        if l == 9 and wide and (last or i > 0 or first_cols_ok):
            names.add("tile_rows512_kernel" if last else "tile_cols512_kernel")
        else:
            names.add("tile_pass_kernel")
    return names


def expected_path(kind, n, batch, plane_offsets, aliasing=False, frame_len=None, stride=None, window=None,
                  sides="one", outputs=(), switches=None):
    """The set of kernel names the call reaches.  kind: complex / real / inverse / ifwd / iinv (interleaved) for
    transforms, spectrum for pdsp_spectrum_f32 and pdsp_spectrum_peaks_f32.  plane_offsets: float offsets of (re_in,
    im_in, re_out, im_out) for transforms, (frames, window) for spectra; None for a missing plane.  window: None,
    ("plan", kind) or ("table", kind).  outputs: a subset of {amp, ph, idx, rec}."""
    sw = dict(DEFAULT_SWITCHES, **(switches or {}))
    L = n.bit_length() - 1
    if kind in ("ifwd", "iinv"):
        return {"fft_stockham_kernel"}
    if kind != "spectrum":
        return _transform_path(kind, L, plane_offsets, aliasing, sw)
    return _spectrum_path(L, batch, plane_offsets, frame_len, stride, window, sides, set(outputs), sw)


def _transform_path(kind, L, offs, aliased, sw):
    re_in, im_in, re_out, im_out = offs
    if kind == "inverse":  # run_complex(im_in, re_in, im_out, re_out): the same planes
        re_in, im_in, re_out, im_out = im_in, re_in, im_out, re_out
    a16 = _a(16, re_in, im_in, re_out, im_out)
    tp = sw["twopass"]
    if L in (15, 16) and tp == 1 and a16 and not aliased:
        return {"fft_paired_kernel"}
    if 15 <= L <= 27 and (tp & 1) and a16:
        if L <= 18:
            ls = [L // 2, L - L // 2]
            return {"tilepass-2"} | _tile_names(ls, True, tp)
        names = {"tilepass-3", "tilepass-3-natural" if tp & 2 else "tilepass-3-perm"}
        if aliased:
            names.add("tilepass-3-scratch2")
        return names | _tile_names(_three(L), True, tp)
    if L > 18:
        # bigfft_rows: N1 = 2^(L - 14) rows; at N = 2^28 N1 == N2 and the first row pass is launch_rows (N = 16384)
        return {"bigfft", "bigfft-n1-rows", "fft_split4_kernel"} if L == 28 and sw["split16k"] else {"bigfft"}
    if L > 14:
        return {"fourstep-fused"}
    if 1 <= L <= 4 and sw["staged_small"] and a16:
        return {"fft_tiny_staged_kernel"}
    if 5 <= L <= 8 and sw["staged_small"] and a16:
        return {"fft_staged_kernel"}
    a16in = _a(16, re_in, im_in)
    if L == 14 and sw["split16k"] and a16in:
        return {"fft_split4_kernel"}
    if L == 13 and sw["split16k"] and (kind == "real" or sw["split16k"] & 2) and a16in:
        return {"fft_split2_kernel"}
    return {"fft_stockham_kernel"}


def _peak_names(bins, outputs):
    names = set()
    if "idx" in outputs:
        names.add("peak_wave_kernel" if bins <= 2048 else "find_peak_kernel")
    if "rec" in outputs:
        names.add("peak_wave_kernel" if bins <= 2048 else "peak_from_rows_kernel")
    return names


FUSED = ("hann", "hamming", "blackman")


def _spectrum_path(L, batch, offs, frame_len, stride, window, sides, outputs, sw):
    n = 1 << L
    f_off, w_off = offs
    used = min(frame_len, n)
    bins = n // 2 + 1 if sides == "one" else n
    if used == 0:
        return {"memset"}
    plan_win = window[1] if window and window[0] == "plan" else None
    rect_plan = plan_win == "rect"
    if L > 14:
        # the packed tile-pass tables (hp_np) exist for 2^15 ... 2^27 only
        if L <= 27 and (sw["twopass"] & 1) and used == n and stride % 4 == 0 and _a(16, f_off, w_off):
            first = 3 if (window is None or rect_plan) else 4
            if plan_win in FUSED and sw["fused_window"]:
                first = 5 if plan_win != "blackman" else 6
            if L == 15 and sw["split16k"]:
                names = {"fft_split4_kernel-packed"}
            elif L == 16 and sw["twopass"] == 1:
                names = {"fft_paired_kernel-packed"}
            else:
                lm = L - 1
                ls = [lm // 2, lm - lm // 2] if lm <= 18 else _three(lm)
                names = {"tilepass_chain-packed"} | _tile_names(ls, False, sw["twopass"])
            return names | {f"packed-first{first}", "split_amp_rows_kernel"} | _peak_names(bins, outputs)
        names = {"bigfft_out<AMP>"} if L > 18 else {"fourstep_ab/c-mode1"}
        if L == 28 and sw["split16k"]:
            names |= {"bigfft-n1-rows", "fft_split4_kernel"}
        return names | _peak_names(bins, outputs)
    if L >= 6:
        fast = _a(8, f_off, w_off) and stride % 2 == 0 and used == n and sides == "one" and "ph" not in outputs
        if fast and not ({"idx", "rec"} & outputs) and L <= 9 and sw["staged_small"] and stride == n \
                and _a(16, f_off, w_off):
            return {"spectrum_staged_kernel"}
        wmode = 1 if window else 0
        if rect_plan:
            wmode = 0
        fuse = 10 <= L <= 14 and sw["fused_window"] and fast
        if fuse and plan_win in FUSED:
            wmode = 3 if plan_win == "blackman" else 2
        if fast and L == 14 and sw["split16k"]:
            return {f"spectrum_dif16k_kernel-w{wmode}" + ("-peak" if "rec" in outputs else "")} | \
                _peak_names(bins, outputs - {"rec"})
        if wmode >= 2 and L == 14:
            wmode = 1
        name = {f"spectrum_packed_kernel-{'FAST' if fast else 'general'}-m{L - 1}-w{wmode}"
                + ("-peak" if "rec" in outputs else "")}
        if L == 14 and not fast:
            name.add("spectrum_packed-16384-general")
        return name | _peak_names(bins, outputs - {"rec"})
    if 1 <= L <= 5 and sw["staged_small"] and used == n and stride == n and "ph" not in outputs \
            and "rec" not in outputs and _a(16, f_off):
        return {"fft_tiny_staged_kernel<AMP>"} | _peak_names(bins, outputs)
    return {"small-complex-(x,0)"} | _peak_names(bins, outputs)


REQUIRED = {
    # transforms
    "fft_tiny_staged_kernel", "fft_stockham_kernel", "fft_staged_kernel", "fft_split2_kernel", "fft_split4_kernel",
    "fft_paired_kernel", "tilepass-2", "tilepass-3", "tilepass-3-perm", "tilepass-3-natural", "tilepass-3-scratch2",
    "tile_pass_kernel", "tile_cols512_kernel", "tile_rows512_kernel", "fourstep-fused", "bigfft", "bigfft-n1-rows",
    # spectra
    "fft_tiny_staged_kernel<AMP>", "small-complex-(x,0)", "spectrum_staged_kernel",
    *[f"spectrum_packed_kernel-{f}-m{m}-w{w}" for f in ("FAST", "general") for m in range(5, 14) for w in (0, 1)],
    *[f"spectrum_packed_kernel-FAST-m{m}-w{w}" for m in range(9, 13) for w in (2, 3)],
    "spectrum_packed_kernel-FAST-m9-w2-peak", "spectrum_packed_kernel-general-m8-w1-peak",
    *[f"spectrum_dif16k_kernel-w{w}{p}" for w in range(4) for p in ("", "-peak")],
    "spectrum_packed-16384-general",
    "packed-first3", "packed-first4", "packed-first5", "packed-first6",
    "fft_split4_kernel-packed", "fft_paired_kernel-packed", "tilepass_chain-packed", "split_amp_rows_kernel",
    "fourstep_ab/c-mode1", "bigfft_out<AMP>",
    "peak_wave_kernel", "find_peak_kernel", "peak_from_rows_kernel", "memset",
}


# ---- the dispatch, asked ----------------------------------------------------------------------------------------

PATH_INFO = 17  # PDSP_DEV_PATH_INFO (include/pdsp_hip_dev.h documents the fields)
ROWS_NAME = {2: "fft_staged_kernel", 3: "fft_stockham_kernel", 4: "fft_split2_kernel", 5: "fft_split4_kernel"}
TILE_NAME = {1: "tile_pass_kernel", 2: "tile_cols512_kernel", 3: "tile_rows512_kernel"}
PEAK_NAME = {1: "peak_wave_kernel", 2: "find_peak_kernel", 4: "peak_from_rows_kernel"}


def path_names(info, n, spectrum=False):
    """expected_path()'s names for the decision the library reports in `info`."""
    (path, rows, n1_rows, n1_square, np_, t0, t1, t2, tile_major, pairs, out_first, fast, wmode, first, fused_peaks,
     peaks, head) = info
    L = n.bit_length() - 1
    tiles = {TILE_NAME[t] for t in (t0, t1, t2)[:np_]}
    peak = {name for bit, name in PEAK_NAME.items() if peaks & bit}
    # the N1-point rows of the general four-step path are named where they run like N2-point rows on fft_split4_kernel
    n1 = {"bigfft-n1-rows", "fft_split4_kernel"} if n1_square and n1_rows == 5 else set()
    if not spectrum:
        assert peak == set() and (rows == path or path not in (3, 4, 5)), list(info)
        if path in (3, 4, 5):
            return {ROWS_NAME[path]}
        if path == 8 and np_ == 2:
            return {"tilepass-2"} | tiles
        if path == 8:
            return {"tilepass-3", "tilepass-3-perm" if tile_major else "tilepass-3-natural"} | tiles | \
                ({"tilepass-3-scratch2"} if pairs == 2 else set())
        if path == 10:
            return {"bigfft"} | n1
        return {{1: "fft_tiny_staged_kernel", 2: "fft_staged_kernel", 7: "fft_paired_kernel", 9: "fourstep-fused"}[path]}
    peak_tag = "-peak" if fused_peaks else ""
    if path == 12:
        names = [{"tilepass_chain-packed"} | tiles, {"fft_split4_kernel-packed"}, {"fft_paired_kernel-packed"}][head]
        return names | {f"packed-first{first}", "split_amp_rows_kernel"} | peak
    if path == 14:
        return {f"spectrum_dif16k_kernel-w{wmode}{peak_tag}"} | peak
    if path == 15:
        names = {f"spectrum_packed_kernel-{'FAST' if fast else 'general'}-m{L - 1}-w{wmode}{peak_tag}"}
        if L == 14 and not fast:
            names.add("spectrum_packed-16384-general")
        return names | peak
    if path == 10:
        return {"bigfft_out<AMP>"} | n1 | peak
    return {{9: "fourstep_ab/c-mode1", 11: "memset", 13: "spectrum_staged_kernel", 16: "fft_tiny_staged_kernel<AMP>",
             17: "small-complex-(x,0)"}[path]} | peak


def asked_path(fn, n, *args, spectrum=False):
    """The names for what the query `fn` reports for a call with these arguments."""
    import ctypes
    info = (ctypes.c_int * PATH_INFO)(*([-1] * PATH_INFO))
    assert fn(*args, info) == 0, _lib().pdsp_last_error()
    return path_names(list(info), n, spectrum)


# ---- buffers ----------------------------------------------------------------------------------------------------

class Buf:
    """`rows` rows of `length` elements, `stride` apart, starting `off` elements past a 4 KiB aligned base that follows
    GUARD elements of `fill`; GUARD more after the last row.  Everything outside the rows holds `fill`."""

    def __init__(self, rows, length, off=0, stride=None, fill=float("nan"), dtype=None):
        import torch
        dtype = dtype or torch.float32
        self.rows, self.length, self.off = rows, length, off
        self.stride = length if stride is None else stride
        self.start = GUARD + off
        span = max(rows - 1, 0) * self.stride + length
        self.flat = torch.full((self.start + span + GUARD,), fill, dtype=dtype, device="cuda:0")
        self.view = torch.as_strided(self.flat, (rows, length), (self.stride, 1), self.start)
        self.ptr = self.flat.data_ptr() + self.flat.element_size() * self.start
        self.fill = fill

    def set(self, a):
        import torch
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(self.flat.dtype))

    def get(self):
        return self.view.cpu().numpy()

    def outside_ok(self):
        """Nothing outside the rows changed (contiguous rows: only the margins are read back)."""
        if self.stride == self.length:
            end = self.start + self.rows * self.length
            parts = [self.flat[:self.start], self.flat[end:]]
            out = np.concatenate([p.cpu().numpy() for p in parts])
        else:
            mask = np.ones(self.flat.numel(), bool)
            idx = self.start + np.arange(self.rows)[:, None] * self.stride + np.arange(self.length)[None, :]
            mask[idx.reshape(-1)] = False
            out = self.flat.cpu().numpy()[mask]
        if np.isnan(self.fill):
            return bool(np.isnan(out).all())
        return bool((out == self.fill).all())


def _lib():
    from pragma_dsp_amd._capi import lib
    return lib


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


class Switches:
    """Development switches for one case, restored in finally (the previous value is what each setter returns)."""

    SETTERS = {"split16k": "pdsp_set_split16k", "twopass": "pdsp_set_twopass", "staged_small": "pdsp_set_staged_small",
               "fused_window": "pdsp_set_fused_window", "real_packed": "pdsp_set_real_packed"}

    def __init__(self, sw):
        self.sw = sw or {}
        self.prev = {}

    def __enter__(self):
        lib = _lib()
        try:
            for k, v in self.sw.items():
                self.prev[k] = getattr(lib, self.SETTERS[k])(v)
        except BaseException:
            self.__exit__()
            raise
        return self

    def __exit__(self, *exc):
        lib = _lib()
        for k, v in self.prev.items():
            getattr(lib, self.SETTERS[k])(v)
        self.prev = {}
        return False


_PLANS = {}


def plan(n):
    from pragma_dsp_amd.batch import BatchedFft
    if n not in _PLANS:
        _PLANS[n] = BatchedFft(n, "cuda:0")
    return _PLANS[n]


@pytest.fixture(scope="module", autouse=True)
def _release_plans():
    import torch
    yield
    for p in _PLANS.values():
        p.close()
    _PLANS.clear()
    torch.cuda.empty_cache()


# ---- inputs -----------------------------------------------------------------------------------------------------

ROW_KINDS = ("gauss", "peaky", "impulse", "const", "zero")


def make_rows(rng, batch, n, complex_, kinds=None, first=0):
    """Rows of the kinds in ROW_KINDS in turn (starting at `first`), each scaled by its own power of two so that a
    mix-up of rows shows.  Returns (re, im or None) rounded to f32, as f64."""
    kinds = kinds or ROW_KINDS
    re = np.zeros((batch, n))
    im = np.zeros((batch, n)) if complex_ else None
    t = np.arange(n)
    for b in range(batch):
        k = kinds[(first + b) % len(kinds)]
        if k == "gauss":
            re[b] = rng.standard_normal(n)
            if complex_:
                im[b] = rng.standard_normal(n)
        elif k == "peaky":
            f = (0.37 * n + 0.31) / n
            re[b] = np.cos(2 * np.pi * f * t + 0.4) + 1e-4 * rng.standard_normal(n)
            if complex_:
                im[b] = np.sin(2 * np.pi * f * t + 0.4) + 1e-4 * rng.standard_normal(n)
        elif k == "impulse":
            re[b, rng.integers(0, n)] = 1.0
            if complex_:
                im[b, rng.integers(0, n)] = -0.75
        elif k == "const":
            re[b] = 0.625
            if complex_:
                im[b] = -1.25
        sc = 2.0 ** ((b % 7) - 3)
        re[b] *= sc
        if complex_:
            im[b] *= sc
    re = re.astype(np.float32).astype(np.float64)
    if complex_:
        im = im.astype(np.float32).astype(np.float64)
    return re, im


PEAK_FLOOR = 1 / 16


def scale(ref, floor=None):
    """Per bin: max(rms(ref), |ref_k|, max|ref| / 16[, floor]) -- see the module docstring."""
    a = np.abs(np.asarray(ref))
    rms = np.sqrt((a ** 2).mean(axis=-1, keepdims=True))
    den = np.maximum(np.maximum(rms, a), PEAK_FLOOR * a.max(axis=-1, keepdims=True, initial=0.0))
    if floor is not None:
        den = np.maximum(den, np.asarray(floor).reshape(-1, 1))
    return den


def row_errors(got, ref, floor=None):
    """max_k |got_k - ref_k| / scale_k per row; rows whose reference is all zeros must be exactly zero (error 0 or
    inf)."""
    got = np.asarray(got)
    ref = np.asarray(ref)
    den = scale(ref, floor)
    d = np.abs(got - ref)
    r = np.where(den > 0, d / np.where(den > 0, den, 1.0), np.where(d == 0, 0.0, np.inf))
    return np.where(np.isnan(d), np.inf, r).max(axis=-1)


class Worst:
    """Worst error per kind in units of log2 N; records one junit property per kind at the end."""

    def __init__(self, record_property, prefix):
        self.rp, self.prefix, self.w = record_property, prefix, {}

    def add(self, kind, n, errs):
        e = float(np.max(errs)) / lg(n)
        self.w[kind] = max(self.w.get(kind, 0.0), e)
        return float(np.max(errs))

    def record(self):
        for k, v in self.w.items():
            self.rp(f"worst_{self.prefix}_{k}", v)


# ---- transforms -------------------------------------------------------------------------------------------------

def run_transform(kind, n, re, im, offs, out_mode="disjoint", switches=None):
    """One raw transform call with planes at `offs` floats (re_in, im_in, re_out, im_out) inside NaN-guarded buffers.
    out_mode: disjoint, inplace (out planes = in planes), overlap (re_out starts half a plane into re_in's buffer).
    Returns (got complex, path names)."""
    import torch
    batch = re.shape[0]
    lib, p = _lib(), plan(n)
    if kind in ("ifwd", "iinv"):
        zin = Buf(batch, 2 * n, offs[0])
        z = np.empty((batch, 2 * n))
        z[:, 0::2], z[:, 1::2] = re, im
        zin.set(z)
        zout = zin if out_mode == "inplace" else Buf(batch, 2 * n, offs[2])
        fn = lib.pdsp_fft_inverse_interleaved_f32 if kind == "iinv" else lib.pdsp_fft_forward_interleaved_f32
        with Switches(switches):
            assert fn(p._h, batch, zin.ptr, zout.ptr, _stream()) == 0
        torch.cuda.synchronize()
        assert zin.outside_ok() and zout.outside_ok(), "write outside the rows"
        g = zout.get().astype(np.float64)
        return g[:, 0::2] + 1j * g[:, 1::2], expected_path(kind, n, batch, offs, switches=switches)
    bre = Buf(batch, n, offs[0])
    bre.set(re)
    bim = None
    if kind != "real":
        bim = Buf(batch, n, offs[1])
        bim.set(im)
    aliased = out_mode != "disjoint"
    im_ptr = bim.ptr if bim is not None else None
    im_off = offs[1] if kind != "real" else None
    checks = []
    if out_mode == "inplace":
        oim = bim if bim is not None else Buf(batch, n, offs[3])
        ore_ptr, read_re = bre.ptr, bre.get
        poffs = (offs[0], im_off, offs[0], offs[1] if kind != "real" else offs[3])
        checks = [bre, oim]
    elif out_mode == "overlap":
        # one buffer holds the real input and, half a plane plus offs[2] floats further on, the real output
        shift = (batch * n) // 2 + offs[2]
        big = Buf(1, batch * n + shift, offs[0])
        big.flat[big.start:big.start + batch * n].copy_(bre.view.reshape(-1))
        bre = big
        oim = Buf(batch, n, offs[3])
        ore_ptr = big.ptr + 4 * shift
        read_re = lambda: big.get()[0, shift:].reshape(batch, n)  # noqa: E731
        poffs = (offs[0], im_off, offs[0] + shift, offs[3])
        checks = [big, oim]
    else:
        ore, oim = Buf(batch, n, offs[2]), Buf(batch, n, offs[3])
        ore_ptr, read_re = ore.ptr, ore.get
        poffs = (offs[0], im_off, offs[2], offs[3])
        checks = [ore, oim]
    s = _stream()
    mirror = expected_path(kind, n, batch, poffs, aliasing=aliased, switches=switches)
    with Switches(switches):
        path = asked_path(lib.pdsp_dev_transform_path_f32, n, p._h, batch, bre.ptr, im_ptr, ore_ptr, oim.ptr,
                          1 if kind == "inverse" else 0)
        assert path == mirror, (kind, n, batch, poffs, out_mode, switches, sorted(path), sorted(mirror))
        if kind == "complex":
            rc = lib.pdsp_fft_forward_complex_f32(p._h, batch, bre.ptr, im_ptr, ore_ptr, oim.ptr, s)
        elif kind == "real":
            rc = lib.pdsp_fft_forward_real_f32(p._h, batch, bre.ptr, ore_ptr, oim.ptr, s)
        else:
            rc = lib.pdsp_fft_inverse_f32(p._h, batch, bre.ptr, im_ptr, ore_ptr, oim.ptr, s)
        torch.cuda.synchronize()
    assert rc == 0, lib.pdsp_last_error()
    for b in checks:
        assert b.outside_ok(), "write outside the output planes"
    got = read_re().astype(np.float64) + 1j * oim.get().astype(np.float64)
    return got, path


def reference_transform(kind, re, im):
    z = re + 1j * im if im is not None else re.astype(np.complex128)
    if kind in ("inverse", "iinv"):
        return np.fft.ifft(z, axis=-1)
    return np.fft.fft(z, axis=-1)


# (id, log2 sizes, batch, kinds, plane offsets re_in / im_in / re_out / im_out in floats, out mode, switches,
#  intended names)
T = ("complex", "real", "inverse")
TRANSFORM_CASES = [
    ("tiny-16B", range(1, 5), 37, T, (0, 4, 8, 12), "disjoint", None, {"fft_tiny_staged_kernel"}),
    ("stockham-n1", range(0, 1), 9, T, (1, 3, 2, 0), "disjoint", None, {"fft_stockham_kernel"}),
    ("stockham-small-off1", range(1, 9), 7, T, (1, 0, 0, 0), "disjoint", None, {"fft_stockham_kernel"}),
    ("stockham-small-off2", range(1, 9), 5, T, (0, 0, 2, 0), "disjoint", None, {"fft_stockham_kernel"}),
    ("stockham-staged-off", range(1, 9), 33, T, (0, 0, 0, 0), "disjoint", {"staged_small": 0}, {"fft_stockham_kernel"}),
    ("staged", range(5, 9), 33, T, (4, 0, 0, 4), "disjoint", None, {"fft_staged_kernel"}),
    ("stockham-512-8192", range(9, 14), 5, ("complex", "inverse"), (0, 0, 0, 0), "disjoint", None,
     {"fft_stockham_kernel"}),
    ("stockham-512-4096-real", range(9, 13), 5, ("real",), (0, 0, 0, 0), "disjoint", None, {"fft_stockham_kernel"}),
    ("interleaved", range(0, 15), 3, ("ifwd", "iinv"), (2, 0, 6, 0), "disjoint", None, {"fft_stockham_kernel"}),
    ("split2-real", range(13, 14), 3, ("real",), (4, 0, 1, 2), "disjoint", None, {"fft_split2_kernel"}),
    ("split2-complex-bit1", range(13, 14), 3, ("complex", "inverse"), (0, 4, 0, 0), "disjoint", {"split16k": 3},
     {"fft_split2_kernel"}),
    ("stockham-8192-real-off1", range(13, 14), 3, ("real",), (1, 0, 0, 0), "disjoint", None, {"fft_stockham_kernel"}),
    # launch_rows decides aligned16 from the input planes only: aligned inputs, outputs off by 1 / 2 floats
    ("split2-out-off", range(13, 14), 3, ("real",), (0, 0, 1, 2), "disjoint", None, {"fft_split2_kernel"}),
    ("split4", range(14, 15), 3, T, (0, 4, 0, 0), "disjoint", None, {"fft_split4_kernel"}),
    ("split4-out-off", range(14, 15), 2, T, (0, 0, 1, 2), "disjoint", None, {"fft_split4_kernel"}),
    ("stockham-16384-in-off", range(14, 15), 2, T, (2, 0, 0, 0), "disjoint", None, {"fft_stockham_kernel"}),
    ("paired", range(15, 17), 3, T, (0, 4, 8, 0), "disjoint", None, {"fft_paired_kernel"}),
    ("tile2", range(15, 19), 3, T, (0, 0, 0, 0), "disjoint", {"twopass": 5}, {"tilepass-2"}),
    ("tile2-inplace", range(15, 19), 2, T, (0, 4, 0, 0), "inplace", None, {"tilepass-2"}),
    ("tile2-overlap", range(15, 17), 2, ("complex", "real"), (0, 4, 4, 0), "overlap", None, {"tilepass-2"}),
    ("tile3-perm", range(19, 24), 2, ("complex", "real", "inverse"), (0, 0, 0, 0), "disjoint", None,
     {"tilepass-3-perm"}),
    ("tile3-natural", range(19, 25, 2), 1, ("complex", "inverse"), (0, 0, 0, 0), "disjoint", {"twopass": 3},
     {"tilepass-3-natural"}),
    ("tile3-512", range(25, 27), 1, ("complex", "real"), (0, 0, 0, 0), "disjoint", None, {"tile_rows512_kernel"}),
    ("tile3-512-natural", range(26, 27), 1, ("inverse",), (0, 0, 0, 0), "disjoint", {"twopass": 3},
     {"tilepass-3-natural"}),
    ("tile3-2p27", range(27, 28), 1, ("complex",), (0, 0, 0, 0), "disjoint", None, {"tile_cols512_kernel"}),
    ("tile3-overlap", range(19, 21), 2, ("complex", "inverse"), (0, 4, 8, 0), "overlap", None,
     {"tilepass-3-scratch2"}),
    ("tile3-inplace", range(21, 22), 1, ("complex",), (0, 4, 0, 0), "inplace", None, {"tilepass-3-scratch2"}),
    ("fourstep-twopass0", range(15, 19), 2, T, (0, 0, 0, 0), "disjoint", {"twopass": 0}, {"fourstep-fused"}),
    ("fourstep-unaligned", range(15, 19), 2, T, (1, 2, 0, 3), "disjoint", None, {"fourstep-fused"}),
    ("bigfft-unaligned", range(19, 22), 1, T, (2, 0, 1, 0), "disjoint", None, {"bigfft"}),
    ("bigfft-inplace", range(19, 20), 2, ("complex", "inverse"), (3, 1, 0, 0), "inplace", None, {"bigfft"}),
    # N = 1 << 28, the largest f32 size: N1 = N2 = 16384, so bigfft_rows' first row pass is launch_rows
    ("bigfft-2p28", range(28, 29), 1, T, (0, 0, 0, 0), "disjoint", None, {"bigfft-n1-rows"}),
]

def _tf_kind(kind):
    return "inv" if kind in ("inverse", "iinv") else "fwd"


@pytest.mark.parametrize("case", TRANSFORM_CASES, ids=[c[0] for c in TRANSFORM_CASES])
def test_transform_paths(record_property, case):
    name, logs, batch, kinds, offs, out_mode, sw, intended = case
    rng = np.random.default_rng(sum(map(ord, name)))
    worst = Worst(record_property, name)
    fails = []
    for L in logs:
        n = 1 << L
        b = batch if n <= 1 << 22 else 1
        for i, kind in enumerate(kinds):
            if out_mode == "inplace" and kind in ("ifwd", "iinv"):
                continue
            re, im = make_rows(rng, b, n, kind != "real", first=L + i)
            got, path = run_transform(kind, n, re, im, offs, out_mode, sw)
            assert intended <= path, (name, L, kind, sorted(path))
            ref = reference_transform(kind, re, im)
            errs = row_errors(got, ref)
            e = worst.add(_tf_kind(kind), n, errs)
            zero = np.all(ref == 0, axis=-1)
            if zero.any():
                assert (got[zero] == 0).all(), (name, L, kind, "zero row not exactly zero")
            if e > bound(_tf_kind(kind), n):
                fails.append((L, kind, e, e / lg(n)))
    worst.record()
    assert not fails, fails


# ---- spectra ----------------------------------------------------------------------------------------------------

def ref_window(n, window, fused):
    """f64 window the reference multiplies by: None, the f32 table (as f64), or the f64 cosine sum when fused."""
    import oracle
    if window is None:
        return None
    kind = window[1]
    w64 = oracle.create_window(kind, n)
    if fused:
        return w64
    return w64.astype(np.float32).astype(np.float64)


def reference_spectrum(frames, n, win, sides):
    """(amplitude, X over the bins returned, scale per bin): spectrum()'s body in f64."""
    x = np.zeros((frames.shape[0], n))
    m = min(frames.shape[1], n)
    x[:, :m] = frames[:, :m]
    if win is not None:
        x = x * win
    if sides == "one":
        X = np.fft.rfft(x, axis=-1)
        sc = np.full(n // 2 + 1, 2.0 / n)
        sc[0] = 1.0 / n
        if n % 2 == 0:
            sc[n // 2] = 1.0 / n
    else:
        X = np.fft.fft(x, axis=-1)
        sc = np.full(n, 1.0 / n)
    return np.abs(X) * sc, X, sc


def _fused(path):
    return any(p.endswith(("-w2", "-w3", "-w2-peak", "-w3-peak")) or p in ("packed-first5", "packed-first6")
               for p in path)


def run_spectrum(n, rows, frame_len, stride, f_off, window, w_off, sides, outputs, switches=None, signal=None):
    """One raw spectrum call.  rows: [batch, min(frame_len, N)] values (f32-exact) placed at `stride` in a NaN buffer
    (or `signal` for overlapping frames); samples past min(frame_len, N) of each row are NaN, so reading them shows.
    window: None, ("plan", kind) or ("table", kind) (a copy at w_off floats).  Returns dict of outputs + path."""
    import torch
    lib, p = _lib(), plan(n)
    batch = rows.shape[0]
    used = min(frame_len, n)
    if signal is not None:
        fb = Buf(1, signal.size, f_off)
        fb.set(signal[None])
    else:
        fb = Buf(batch, max(frame_len, 1), f_off, stride=stride) if batch else Buf(1, 1, f_off)
        full = np.full((batch, max(frame_len, 1)), np.nan)
        full[:, :used] = rows[:, :used]
        fb.set(full)
    wptr, wb = None, None
    if window is not None and window[0] == "plan":
        wptr = p.window(window[1]).data_ptr()
        w_off = 0
    elif window is not None:
        import oracle
        wb = Buf(1, n, w_off)
        wb.set(oracle.create_window(window[1], n).astype(np.float32)[None])
        wptr = wb.ptr
    bins = n // 2 + 1 if sides == "one" else n
    out = {}
    amp = Buf(batch, bins) if "amp" in outputs else None
    ph = Buf(batch, bins, 1) if "ph" in outputs else None
    idx = Buf(batch, 1, 0, fill=SENT_I32, dtype=torch.int32) if "idx" in outputs else None
    rec = Buf(batch, 4, 0, fill=SENT_I32, dtype=torch.int32) if "rec" in outputs else None
    ptr = lambda b: b.ptr if b is not None else None  # noqa: E731
    two = 1 if sides == "two" else 0
    mirror = expected_path("spectrum", n, batch, (f_off, w_off if window else None), frame_len=frame_len, stride=stride,
                           window=window, sides=sides, outputs=outputs, switches=switches)
    with Switches(switches):
        path = asked_path(lib.pdsp_dev_spectrum_path_f32, n, p._h, batch, fb.ptr, frame_len, stride, wptr, two, ptr(amp),
                          ptr(ph), ptr(idx), ptr(rec), SR if rec is not None else 1.0, spectrum=True)
        assert path == mirror, (n, batch, frame_len, stride, f_off, window, w_off, sides, sorted(outputs), switches,
                                sorted(path), sorted(mirror))
        if rec is not None:
            rc = lib.pdsp_spectrum_peaks_f32(p._h, batch, fb.ptr, frame_len, stride, wptr, two, SR, ptr(amp), ptr(ph),
                                             rec.ptr, _stream())
        else:
            rc = lib.pdsp_spectrum_f32(p._h, batch, fb.ptr, frame_len, stride, wptr, two, ptr(amp), ptr(ph), ptr(idx),
                                       _stream())
        torch.cuda.synchronize()
    assert rc == 0, lib.pdsp_last_error()
    for k, b in (("amp", amp), ("ph", ph), ("idx", idx), ("rec", rec)):
        if b is not None:
            assert b.outside_ok(), f"{k}: write outside the output rows"
            out[k] = b.get()
    out["path"] = path
    return out


def check_spectrum(worst, n, frames, out, window, sides, ctx):
    """Amplitude, phase and peaks of one call against the reference; returns the list of failures."""
    path = out["path"]
    fused = _fused(path)
    amp_ref, X, sc = reference_spectrum(frames, n, ref_window(n, window, fused), sides)
    b_amp = bound("amp", n)
    fails = []
    rms = np.sqrt((amp_ref ** 2).mean(axis=-1))
    zero = rms == 0
    # a fused cosine sum is a few f32 ulps off in absolute terms: where the window is small its relative error is
    # large, so those rows are also measured against the rms of the unwindowed frame's amplitude
    floor = None
    if fused:
        raw, _, _ = reference_spectrum(frames, n, None, sides)
        floor = np.sqrt((raw ** 2).mean(axis=-1))
    den = scale(amp_ref, floor)
    zero_in = (frames == 0).all(axis=-1)  # +0 samples (a window of zeros makes signed zeros: no phase asserted)
    if "amp" in out:
        a = out["amp"].astype(np.float64)
        assert not np.isnan(a).any(), (ctx, "NaN left in amplitude rows")
        errs = row_errors(a, amp_ref, floor)
        e = worst.add("amp", n, errs)
        if e > b_amp:
            fails.append((ctx, "amp", e / lg(n)))
        if zero.any():
            assert (a[zero] == 0).all(), ctx
    if "ph" in out:
        ph = out["ph"].astype(np.float64)
        assert not np.isnan(ph).any(), (ctx, "NaN left in phase rows")
        mag = np.abs(X) * sc
        ok = mag >= 1e-3 * rms[:, None]
        d = np.abs(np.angle(np.exp(1j * (ph - np.angle(X)))))
        lim = PHASE_C * b_amp * den / np.where(ok, mag, 1.0)
        if (d[ok] > lim[ok]).any():
            fails.append((ctx, "phase", float((d / lim)[ok].max())))
        worst.w["phase_in_bound"] = max(worst.w.get("phase_in_bound", 0.0), float((d / lim)[ok].max(initial=0)))
        if zero_in.any():
            assert (ph[zero_in] == 0).all(), (ctx, "phase of an all-zero row")
    for key in ("idx", "rec"):
        if key not in out:
            continue
        got = out[key][:, 0].astype(np.int64)
        for r in range(frames.shape[0]):
            g = int(got[r])
            A = amp_ref[r]
            cand = A[1:]
            if zero[r] or cand.max(initial=0) <= 0:
                assert g == 0, (ctx, key, r, g)
                continue
            kr = 1 + int(np.argmax(cand))
            tie = 0 < g < A.size and A[g] >= A[kr] - 2 * b_amp * den[r, kr]
            mirror = sides == "two" and g == n - kr
            assert g == kr or mirror or tie, (ctx, key, r, g, kr)
        if key == "rec":
            rec = out["rec"]
            f = rec[:, 1:].view(np.float32)
            freq = np.float32(SR / n)
            assert np.array_equal(f[:, 0], got.astype(np.float32) * freq), (ctx, "frequency")
            A_at = amp_ref[np.arange(got.size), got]
            if "amp" in out:
                assert np.array_equal(f[:, 1], out["amp"][np.arange(got.size), got]), (ctx, "record amplitude")
            dg = den[np.arange(got.size), got]
            da = np.abs(f[:, 1] - A_at) / np.where(rms > 0, dg, 1.0)
            if (da > b_amp).any():
                fails.append((ctx, "rec.amplitude", float(da.max())))
            if "ph" in out:
                assert np.array_equal(f[:, 2], out["ph"][np.arange(got.size), got]), (ctx, "record phase")
            Xg = X[np.arange(got.size), got]
            okr = np.abs(Xg) * sc[got] >= 1e-3 * rms
            dp = np.abs(np.angle(np.exp(1j * (f[:, 2] - np.angle(Xg)))))
            lim = PHASE_C * b_amp * dg / np.where(okr, np.abs(Xg) * sc[got], 1.0)
            if (dp[okr] > lim[okr]).any():
                fails.append((ctx, "rec.phase", float((dp / lim)[okr].max())))
            assert (f[zero_in, 2] == 0).all() and (f[zero, 1] == 0).all(), (ctx, "record of an all-zero row")
    return fails


# (id, log2 sizes, batch, frame mode, stride mode, frames offset, windows, window offset, sides, output sets,
#  switches, intended name prefix)
#   frame mode: full (N), part (about 2N/3), long (N + 5), zero (0); stride mode: len (= frame length), gap<k>
#   (frame length + k), hop<k> (overlapping frames N/k apart)
A, P, I, R = ("amp",), ("amp", "ph"), ("amp", "idx"), ("rec",)
W_ALL = (None, ("plan", "rect"), ("plan", "hann"), ("table", "hamming"))
W_FUSE = (("plan", "hann"), ("plan", "hamming"), ("plan", "blackman"))
SPEC_CASES = [
    ("tiny-amp", range(1, 6), 37, "full", "len", 0, W_ALL, 0, ("one", "two"), (A, I), None),
    ("small-x0-n1", range(0, 1), 9, "full", "len", 1, (None,), 0, ("one", "two"), (A, P, I, R), None),
    ("small-x0", range(1, 6), 11, "full", "len", 0, W_ALL, 0, ("one", "two"), (P, R, ("rec", "amp", "ph")), None),
    ("small-x0-part", range(1, 6), 5, "part", "gap3", 1, (None, ("table", "hann")), 1, ("one",), (A, I), None),
    ("small-x0-hop", range(2, 6), 6, "full", "hop2", 2, (("plan", "hann"),), 0, ("two",), (P,), None),
    ("small-x0-long", range(1, 6), 4, "long", "len", 0, (None,), 0, ("one",), (A,), None),
    ("staged", range(6, 10), 37, "full", "len", 0, W_ALL, 0, ("one",), (A,), None),
    ("packed-fast", range(6, 15), 5, "full", "len", 0, (None, ("table", "hann")), 0, ("one",), (A, I, R), None),
    ("packed-fast-fused", range(10, 14), 5, "full", "len", 0, W_FUSE, 0, ("one",), (A, R, ("rec", "amp")), None),
    ("packed-fast-stride", range(6, 14), 3, "full", "gap2", 2, (None, ("plan", "hann")), 0, ("one",), (A,), None),
    ("packed-general-phase", range(6, 15), 3, "full", "len", 0, (None, ("table", "blackman")), 0, ("one",),
     (P, ("rec", "amp", "ph")), None),
    ("packed-general-two", range(6, 15), 3, "full", "len", 0, (None, ("plan", "hamming")), 0, ("two",), (A, R),
     None),
    ("packed-general-part", range(6, 15), 3, "part", "gap1", 1, (("table", "hann"),), 1, ("one",), (A, I), None),
    ("packed-general-long", range(6, 12), 3, "long", "len", 0, (None,), 0, ("one",), (A,), None),
    ("packed-hop", range(6, 15), 5, "full", "hop4", 0, (("plan", "hann"),), 0, ("one",), (A, R), None),
    # the FAST predicate with a window table at an odd float offset
    ("packed-win-odd", range(6, 15), 3, "full", "len", 0, (("table", "hann"),), 1, ("one",), (A,), None),
    ("dif16k", range(14, 15), 3, "full", "len", 0, W_ALL + (("plan", "blackman"),), 0, ("one",), (A, R, I), None),
    ("packed-16384-split0", range(14, 15), 3, "full", "len", 0, (None, ("plan", "hann")), 0, ("one",), (A,),
     {"split16k": 0}),
    ("packed-fused-off", range(10, 15), 3, "full", "len", 0, (("plan", "blackman"),), 0, ("one",), (A,),
     {"fused_window": 0}),
    ("staged-off", range(6, 10), 5, "full", "len", 0, (None,), 0, ("one",), (A,), {"staged_small": 0}),
    ("tiny-off", range(1, 6), 5, "full", "len", 0, (None,), 0, ("one",), (A,), {"staged_small": 0}),
    ("chain-2p15-2p18", range(15, 19), 2, "full", "len", 0, W_ALL + (("plan", "blackman"),), 0, ("one",), (A, R),
     None),
    ("chain-ph-two", range(15, 18), 2, "full", "len", 0, (("plan", "hann"),), 0, ("one", "two"), (P, I), None),
    ("chain-twopass5", range(15, 17), 2, "full", "len", 0, (None, ("plan", "hann")), 0, ("one",), (A,),
     {"twopass": 5, "split16k": 0}),
    ("chain-3pass", range(19, 24), 1, "full", "len", 0, (None, ("plan", "hann"), ("table", "blackman")), 0, ("one",),
     (A, ("rec", "amp")), None),
    ("chain-3pass-natural", range(19, 21), 1, "full", "len", 0, (("plan", "hamming"),), 0, ("one",), (A,),
     {"twopass": 3}),
    ("chain-512", range(20, 28, 7), 1, "full", "len", 0, (("plan", "blackman"),), 0, ("one",), (A,), None),
    ("fourstep-spec-part", range(15, 19), 2, "part", "len", 0, (None, ("plan", "hann")), 0, ("one", "two"),
     (P, I, R), None),
    ("fourstep-spec-unaligned", range(15, 19), 2, "full", "len", 2, (("plan", "hamming"),), 0, ("one",), (A,), None),
    ("fourstep-spec-stride", range(15, 19), 2, "full", "gap2", 0, (None,), 0, ("one",), (A,), None),
    ("fourstep-spec-twopass0", range(15, 17), 2, "full", "len", 0, (None,), 0, ("one",), (A,), {"twopass": 0}),
    ("bigfft-spec", range(19, 22), 1, "part", "len", 0, (("plan", "hann"),), 0, ("one",), (P, R), None),
    ("bigfft-spec-stride", range(19, 20), 2, "full", "gap1", 0, (None,), 0, ("one",), (A, I), None),
    # N = 1 << 28: no packed tile-pass tables, so whole aligned frames take bigfft AMP too (launch_rows N1 pass)
    ("bigfft-spec-2p28", range(28, 29), 1, "full", "len", 0, (("plan", "hann"),), 0, ("one",), (A, I), None),
    ("memset", range(0, 15, 7), 3, "zero", "gap1", 0, (None,), 0, ("one", "two"), (P, I, R), None),
]


# the kernel (name prefix) each spectrum case is there to reach, asserted on every call
SPEC_WANT = {
    "tiny-amp": ("fft_tiny_staged_kernel<AMP>",), "small-x0-n1": ("small-complex",), "small-x0": ("small-complex",),
    "small-x0-part": ("small-complex",), "small-x0-hop": ("small-complex",), "small-x0-long": ("small-complex",),
    "staged": ("spectrum_staged_kernel",),
    "packed-fast": ("spectrum_packed_kernel-FAST", "spectrum_staged_kernel", "spectrum_dif16k_kernel"),
    "packed-fast-fused": ("spectrum_packed_kernel-FAST",), "packed-fast-stride": ("spectrum_packed_kernel-FAST",),
    "packed-general-phase": ("spectrum_packed_kernel-general",),
    "packed-general-two": ("spectrum_packed_kernel-general",),
    "packed-general-part": ("spectrum_packed_kernel-general",),
    "packed-general-long": ("spectrum_packed_kernel-general",),
    "packed-hop": ("spectrum_packed_kernel-FAST", "spectrum_dif16k_kernel"),
    "packed-win-odd": ("spectrum_packed_kernel-general",), "dif16k": ("spectrum_dif16k_kernel",),
    "packed-16384-split0": ("spectrum_packed_kernel-FAST-m13",),
    "packed-fused-off": ("spectrum_packed_kernel-FAST", "spectrum_dif16k_kernel-w1"),
    "staged-off": ("spectrum_packed_kernel-FAST",), "tiny-off": ("small-complex",),
    "chain-2p15-2p18": ("split_amp_rows_kernel",), "chain-ph-two": ("split_amp_rows_kernel",),
    "chain-twopass5": ("tilepass_chain-packed",), "chain-3pass": ("tilepass_chain-packed",),
    "chain-3pass-natural": ("tilepass_chain-packed",), "chain-512": ("tilepass_chain-packed",),
    "fourstep-spec-part": ("fourstep_ab/c-mode1",), "fourstep-spec-unaligned": ("fourstep_ab/c-mode1",),
    "fourstep-spec-stride": ("fourstep_ab/c-mode1",), "fourstep-spec-twopass0": ("fourstep_ab/c-mode1",),
    "bigfft-spec": ("bigfft_out<AMP>",), "bigfft-spec-stride": ("bigfft_out<AMP>",),
    "bigfft-spec-2p28": ("bigfft-n1-rows",), "memset": ("memset",),
}


def _frame_geometry(n, frame, stride_mode):
    length = {"full": n, "part": max(n - n // 3 - 1, 1), "long": n + 5, "zero": 0}[frame]
    if stride_mode == "len":
        return length, max(length, 1), None
    if stride_mode.startswith("gap"):
        return length, max(length, 1) + int(stride_mode[3:]), None
    return length, max(n // int(stride_mode[3:]), 1), "hop"


def spectrum_rows(rng, batch, n, length, stride, hop, first):
    """(rows [batch, used] f32-exact as f64, the signal for overlapping frames or None)."""
    used = min(length, n)
    if hop:
        sig = rng.standard_normal((batch - 1) * stride + used)
        sig[: used // 2] += 3 * np.cos(2 * np.pi * 0.21 * np.arange(used // 2))
        sig = sig.astype(np.float32).astype(np.float64)
        rows = np.stack([sig[b * stride:b * stride + used] for b in range(batch)])
        return rows, sig
    re, _ = make_rows(rng, batch, max(used, 1), False, first=first)
    return re[:, :used], None


@pytest.mark.parametrize("case", SPEC_CASES, ids=[c[0] for c in SPEC_CASES])
def test_spectrum_paths(record_property, case):
    name, logs, batch, frame, smode, f_off, windows, w_off, sidess, outsets, sw = case
    rng = np.random.default_rng(sum(map(ord, name)) + 7)
    worst = Worst(record_property, name)
    fails = []
    for L in logs:
        n = 1 << L
        for wi, window in enumerate(windows):
            if n == 1 and window is not None:
                continue
            for sides in sidess:
                for oi, outs in enumerate(outsets):
                    length, stride, hop = _frame_geometry(n, frame, smode)
                    rows, sig = spectrum_rows(rng, batch, n, length, stride, hop, L + wi + oi)
                    out = run_spectrum(n, rows, length, stride, f_off, window, w_off, sides, set(outs), sw, sig)
                    ctx = (name, L, window, sides, outs, sorted(out["path"]))
                    assert any(p.startswith(w) for p in out["path"] for w in SPEC_WANT[name]), ctx
                    if length == 0:
                        for k in ("amp", "ph", "idx"):
                            if k in out:
                                assert (out[k] == 0).all(), ctx
                        if "rec" in out:
                            assert (out["rec"] == 0).all(), ctx
                        continue
                    fails += check_spectrum(worst, n, rows, out, window, sides, ctx)
    worst.record()
    assert not fails, fails


def test_path_table_reaches_every_path():
    """The expected paths of every case in the two tables, without running them: each REQUIRED name is reached."""
    seen = set()
    for name, logs, batch, kinds, offs, out_mode, sw, intended in TRANSFORM_CASES:
        for L in logs:
            for kind in kinds:
                if kind == "real":
                    o = (offs[0], None, offs[2], offs[3])
                    if out_mode == "inplace":
                        o = (offs[0], None, offs[0], offs[3])
                else:
                    o = offs if out_mode != "inplace" else (offs[0], offs[1], offs[0], offs[1])
                if out_mode == "overlap":
                    shift = ((batch if L <= 22 else 1) << L) // 2 + offs[2]
                    o = (o[0], o[1], offs[0] + shift, offs[3])
                path = expected_path(kind, 1 << L, batch, o, aliasing=out_mode != "disjoint", switches=sw)
                assert intended <= path, (name, L, kind, sorted(path))
                seen |= path
    for name, logs, batch, frame, smode, f_off, windows, w_off, sidess, outsets, sw in SPEC_CASES:
        for L in logs:
            n = 1 << L
            length, stride, _ = _frame_geometry(n, frame, smode)
            for window in windows:
                if n == 1 and window is not None:
                    continue
                wo = (0 if window[0] == "plan" else w_off) if window else None
                for sides in sidess:
                    for outs in outsets:
                        path = expected_path("spectrum", n, batch, (f_off, wo), frame_len=length, stride=stride,
                                             window=window, sides=sides, outputs=set(outs), switches=sw)
                        assert any(p.startswith(w) for p in path for w in SPEC_WANT[name]), (name, L, window, path)
                        seen |= path
    missing = REQUIRED - seen
    assert not missing, sorted(missing)


def test_reference_spectrum_matches_the_oracle(oracle_mod):
    """reference_spectrum() restates the oracle's scaling: pinned at a few small N, both sides, with a window."""
    rng = np.random.default_rng(5)
    for n in (1, 2, 8, 64, 1024):
        x = rng.standard_normal((3, n)).astype(np.float32).astype(np.float64)
        for sides in ("one", "two"):
            for kind in (None, "hann"):
                w = oracle_mod.create_window(kind, n) if kind else None
                amp, _, _ = reference_spectrum(x, n, w, sides)
                want, _, _ = oracle_mod.Plan(n).spectrum_batch(x, window=w, two_sided=sides == "two")
                assert np.abs(amp - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), (n, sides, kind)


# ---- bitwise invariances ----------------------------------------------------------------------------------------

INV_T = [(3, 37, (0, 4, 8, 12)), (6, 33, (4, 0, 0, 4)), (7, 70, (1, 0, 0, 0)), (10, 9, (0, 0, 0, 0)),
         (13, 5, (0, 0, 0, 0)), (14, 3, (0, 0, 0, 0)), (16, 3, (0, 0, 0, 0)), (20, 2, (0, 0, 0, 0))]
INV_S = [(4, 300, None, "one"), (5, 130, ("table", "hann"), "two"), (7, 200, None, "one"),
         (8, 33, ("plan", "hann"), "one"), (11, 9, ("plan", "blackman"), "one"), (12, 9, None, "two"),
         (14, 5, ("plan", "hann"), "one"), (15, 3, ("plan", "hamming"), "one"), (20, 2, None, "one")]


def _transform_once(n, re, im, offs, kind="complex"):
    got, _ = run_transform(kind, n, re, im, offs)
    return got


def _spectrum_once(n, rows, window, sides, outs=("amp",)):
    out = run_spectrum(n, rows, n, n, 0, window, 0, sides, set(outs))
    return out["amp"]


@pytest.mark.parametrize("L,batch,offs", INV_T, ids=[f"N{1 << c[0]}" for c in INV_T])
def test_transform_row_position_scaling_and_isolation(L, batch, offs):
    """A row gives the same bits alone and at several positions in a batch (dead rows in the last workgroup
    included); scaling a row by 2^k scales its output bit for bit; NaN / Inf rows leave every other row's bits."""
    n = 1 << L
    rng = np.random.default_rng(L)
    re, im = make_rows(rng, batch, n, True, kinds=("gauss", "peaky", "impulse", "const"))
    base = _transform_once(n, re, im, offs)
    for b in sorted({0, 1, batch // 2, batch - 1}):
        alone = _transform_once(n, re[b:b + 1], im[b:b + 1], offs)
        assert np.array_equal(alone[0], base[b]), ("alone", n, b)
    rolled = _transform_once(n, np.roll(re, 1, axis=0), np.roll(im, 1, axis=0), offs)
    assert np.array_equal(rolled, np.roll(base, 1, axis=0)), ("rolled", n)
    for k in (-20, 17):
        sc = _transform_once(n, np.ldexp(re, k), np.ldexp(im, k), offs)
        want = np.ldexp(base.real, k) + 1j * np.ldexp(base.imag, k)
        assert np.array_equal(sc, want), ("scale", n, k)
    bad_re, bad_im = re.copy(), im.copy()
    bad_re[batch // 2, n // 3] = np.nan
    if batch > 2:
        bad_im[batch - 1, n - 1] = np.inf
    got = _transform_once(n, bad_re, bad_im, offs)
    keep = np.ones(batch, bool)
    keep[[batch // 2, batch - 1] if batch > 2 else [batch // 2]] = False
    assert np.array_equal(got[keep], base[keep]), ("isolation", n)
    assert not np.isfinite(got[batch // 2]).all()


@pytest.mark.parametrize("L,batch,window,sides", INV_S, ids=[f"N{1 << c[0]}" for c in INV_S])
def test_spectrum_row_position_scaling_and_isolation(L, batch, window, sides):
    """The same invariances for amplitude rows: alone == in the batch, 2^k in == 2^k out, NaN / Inf isolated."""
    n = 1 << L
    rng = np.random.default_rng(100 + L)
    rows, _ = make_rows(rng, batch, n, False, kinds=("gauss", "peaky", "impulse", "const"))
    base = _spectrum_once(n, rows, window, sides)
    for b in sorted({0, 1, batch // 2, batch - 1}):
        assert np.array_equal(_spectrum_once(n, rows[b:b + 1], window, sides)[0], base[b]), ("alone", n, b)
    assert np.array_equal(_spectrum_once(n, np.roll(rows, 3, axis=0), window, sides), np.roll(base, 3, axis=0))
    for k in (-20, 17):
        got = _spectrum_once(n, np.ldexp(rows, k), window, sides)
        assert np.array_equal(got, np.ldexp(base, k)), ("scale", n, k)
    bad = rows.copy()
    bad[batch // 2, n // 3] = np.nan
    if batch > 2:
        bad[batch - 1, 0] = -np.inf
    got = _spectrum_once(n, bad, window, sides)
    keep = np.ones(batch, bool)
    keep[[batch // 2, batch - 1] if batch > 2 else [batch // 2]] = False
    assert np.array_equal(got[keep], base[keep]), ("isolation", n)
    assert not np.isfinite(got[batch // 2]).all()


# ---- the f32 magnitude's range ----------------------------------------------------------------------------------
# mag() squares in f32 (include/pdsp_hip.h): re^2 + im^2 overflows above |X| = sqrt(FLT_MAX) = 1.8e19 and leaves the
# normal range below sqrt(FLT_MIN) = 1.1e-19.  The fused spectrum stores square either the bin X or the bin times
# s / 2 (amplitude / 2), so their range is |X_k| <= 1.8e19 and amplitude >= 2.2e-19.  Just inside both ends (|X| = 2^63,
# amplitude 2^-61 at the edge bins) the amplitude rows are the unit case scaled by a power of two.


@pytest.mark.parametrize("edge", ["upper", "lower"])
def test_magnitude_range_edges(edge):
    import torch
    lib = _lib()
    # stand-alone magnitude: |(re, im)| at 2^63 or 2^-62 at many angles, within 1 ulp of the f64 value
    a = 2.0 ** 63 if edge == "upper" else 2.0 ** -62
    ang = np.linspace(0, 2 * np.pi, 4097)
    re = (a * np.cos(ang)).astype(np.float32)
    im = (a * np.sin(ang)).astype(np.float32)
    want = np.hypot(re.astype(np.float64), im.astype(np.float64))
    dre, dim = torch.from_numpy(re).cuda(), torch.from_numpy(im).cuda()
    out = Buf(1, re.size)
    assert lib.pdsp_magnitude_f32(re.size, dre.data_ptr(), dim.data_ptr(), out.ptr, _stream()) == 0
    torch.cuda.synchronize()
    assert out.outside_ok()
    got = out.get()[0].astype(np.float64)
    ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
    assert (np.abs(got - want) <= ulp).all(), (edge, float((np.abs(got - want) / ulp).max()))
    # fused spectrum stores: impulses, |X_k| = height at every bin; the rows of height 1 scaled by 2^k must come back
    seen = set()
    for n in (2, 16, 32, 64, 512, 1024, 8192, 16384, 1 << 15, 1 << 16, 1 << 17, 1 << 19):
        for sides, outs, window in (("one", {"amp"}, None), ("one", {"amp", "ph"}, None), ("two", {"rec", "amp"}, None),
                                    ("one", {"amp"}, ("plan", "hann")), ("one", {"amp", "idx"}, ("plan", "rect"))):
            if window and n < 1024:
                continue
            # a window halves the row-0 impulse (n / 4) and scales the edge bins: two more binades at the lower end
            k = 63 if edge == "upper" else int(np.log2(n)) - 61 + (2 if window else 0)
            rows = np.zeros((2, n))
            rows[0, (n // 4 if window else 3) % n] = 1.0
            rows[1, (n // 2 + 1) % n] = -1.0
            unit = run_spectrum(n, rows, n, n, 0, window, 0, sides, outs)
            big = run_spectrum(n, np.ldexp(rows, k), n, n, 0, window, 0, sides, outs)
            seen |= big["path"]
            want = np.ldexp(unit["amp"].astype(np.float64), k)
            got = big["amp"].astype(np.float64)
            if window is None:  # every bin of an impulse is inside the range; a window's zeros are not
                ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
                assert (np.abs(got - want) <= ulp).all(), (edge, n, sides, outs, sorted(big["path"]))
                if edge == "upper":
                    assert np.array_equal(got, want), (edge, n, sides, sorted(big["path"]))
            else:
                amp_ref, _, _ = reference_spectrum(np.ldexp(rows, k), n, ref_window(n, window, True), sides)
                assert row_errors(got, amp_ref).max() <= bound("amp", n), (edge, n, window, sorted(big["path"]))
    assert {"fft_tiny_staged_kernel<AMP>", "spectrum_staged_kernel", "spectrum_dif16k_kernel-w0",
            "split_amp_rows_kernel", "small-complex-(x,0)"} <= seen

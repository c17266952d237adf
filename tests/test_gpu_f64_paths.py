"""The f64 transform and spectrum kernels path by path, against long-double references of the exact f64 inputs.

The dispatcher (pdsp_dispatch.inc: pick_transform, pick_spectrum and the launchers that switch on their result;
run_interleaved) picks among the f64 kernel forms by size, batch, plane alignment (offsets of 1, 2 and 4 doubles give
8-, 16- and 32-byte alignment), aliasing, frame length, stride, window, sides, requested outputs and three development
switches.  expected_path_f64() below restates those predicates for T = double, independently.  Before every call the
library itself is asked (pdsp_dev_transform_path_f64 / pdsp_dev_spectrum_path_f64, on the call's own pointers and
under its switch values); path_names_f64() puts the answer into the same vocabulary and the two sets must be EQUAL.
Every case then asserts the path it names on the library's answer, and tests/test_f64_paths_cpu.py checks (without a
GPU) that the tables reach each name in REQUIRED_F64.  f64 has no peak
records (pdsp_spectrum_peaks_f32 only), so of the three peak kernels it reaches peak_wave_kernel and find_peak_kernel.

References: numpy.fft on np.longdouble input, which numpy 2.x computes in x86 80-bit precision (complex256, eps
1.1e-19); ld_fft() refuses anything else, so a bound near 1e-16 is never anchored to an f64 reference with the
kernel's own error.  The comparison splits the reference into f64 hi + lo parts and takes (got - hi) - lo, so the
reference's rounding to f64 is not part of what is measured either.  Spectrum cases apply the scaling of spectrum()
(s_edge = 1/N at bins 0 and N/2 one-sided, s_mid = 2/N elsewhere; 1/N two-sided).  A window is compared as the plan's
f64 table (pdsp_plan_window_f64: f64 has no fused cosine-sum window), and that table is pinned once against the cosine
sum evaluated in long double.  At N = 2^26 one long-double reference row takes about 1 GiB and 20 s on the host.

Metric, per row (the f32 file's): max_k |got_k - ref_k| / scale_k, scale_k = max(rms(ref), |ref_k|, max|ref| / 16).
Phase is checked where |X_k| >= 1e-3 rms, within PHASE_C * bound * scale_k / |X_k| rad; up to N = 2^21 (the sizes
test_gpu_f64_dispatch.py runs) that limit is asserted to be tighter than its 1e-9 rad at every bin it covers (the
largest limit per case is recorded as `worst_*_phase_limit`).  Inputs per case: Gaussian rows, an
off-bin sinusoid plus 1e-4 noise, an impulse at a random position, a constant and an all-zero row, each scaled by its
own power of two.

Bounds are TOL[kind] x log2 N (log2 N taken as 1 for N = 1), at 2.4-3x the worst error measured on an MI355X across
this file (recorded per case as `worst_*` junit properties, in units of log2 N; the inputs are seeded):
  forward transforms  1.98e-16 x log2 N (fft_real_kernel, 16384; family median 1.0e-16), bound 5e-16 x log2 N;
  inverse transforms  1.64e-16 x log2 N (fft_stockham_kernel, N <= 128), bound 4.5e-16 x log2 N;
  amplitude rows      2.27e-16 x log2 N (spectrum_packed_kernel general, table window), bound 6e-16 x log2 N;
  phase               0.85 of its bound at most; its limit up to N = 2^21 is 1.4e-10 rad at most.
The bigfft sizes (2^18 ... 2^26) measure 0.9-1.4e-16 x log2 N: no path is out of line with the family.
test_gpu_f64_dispatch.py's 1e-14 / 1e-13 of max|X| is 50-100x above these bounds for a Gaussian row.
"""
import numpy as np
import pytest

from test_gpu_f32_paths import Buf, Switches, Worst, lg, scale, SENT_I32, PATH_INFO, ROWS_NAME, PEAK_NAME

pytestmark = pytest.mark.gpu

TOL = {"fwd": 5e-16, "inv": 4.5e-16, "amp": 6e-16}  # x log2 N
PHASE_C = 0.5
OLD_PHASE_TOL = 1e-9  # test_gpu_f64_dispatch.py's phase bound, which it applies up to N = 2^21
OLD_PHASE_MAX_N = 1 << 21


def bound(kind, n):
    return TOL[kind] * lg(n)


# ---- the dispatch, restated -------------------------------------------------------------------------------------

DEFAULT_SWITCHES = {"split16k": 1, "staged_small": 1, "real_packed": 1}
MAX_LOG2N = 13  # kMaxLog2N_f64: the single-pass limit (N2 of the four-step paths)
MAX_LOG2N1 = 4  # kMaxLog2N1: fused four-step columns


def _a(nbytes, *offs):
    """Are the planes at these double offsets (past a 4 KiB aligned base) multiples of nbytes?  None = no plane."""
    return all(o is None or (8 * o) % nbytes == 0 for o in offs)


def _bigfft_rows(L, sw):
    """bigfft_rows: N1 = 2^(L - 13) rows first (three forms), then N2 = 8192-point rows (launch_rows, aligned scratch)."""
    l1 = L - MAX_LOG2N
    if l1 == MAX_LOG2N:
        first = {"bigfft-n1-split2", "fft_split2_kernel" if sw["split16k"] else "fft_stockham_kernel"}
    elif l1 <= 7 and sw["staged_small"]:
        first = {"bigfft-n1-staged", "fft_staged_kernel"}
    else:
        first = {"bigfft-n1-stockham-tw1", "fft_stockham_kernel"}
    return first | {"fft_split2_kernel" if sw["split16k"] else "fft_stockham_kernel"}


def expected_path_f64(kind, n, batch, plane_offsets, aliasing=False, frame_len=None, stride=None, window=None,
                      sides="one", outputs=(), switches=None):
    """The set of kernel names the call reaches.  kind: complex / real / inverse / ifwd / iinv (interleaved) for
    transforms, spectrum for pdsp_spectrum_f64.  plane_offsets: double offsets of (re_in, im_in, re_out, im_out) for
    transforms, (frames, window) for spectra; None for a missing plane.  window: None, ("plan", kind) or ("table",
    kind).  outputs: a subset of {amp, ph, idx}."""
    sw = dict(DEFAULT_SWITCHES, **(switches or {}))
    L = n.bit_length() - 1
    if kind in ("ifwd", "iinv"):
        assert L <= MAX_LOG2N
        return {"fft_stockham_kernel"}
    if kind != "spectrum":
        return _transform_path(kind, L, batch, plane_offsets, aliasing, sw)
    return _spectrum_path(L, batch, plane_offsets, frame_len, stride, window, sides, set(outputs), sw)


def _transform_path(kind, L, batch, offs, aliased, sw):
    re_in, im_in, re_out, im_out = offs
    if kind == "inverse":  # run_complex(im_in, re_in, im_out, re_out): the same planes
        re_in, im_in, re_out, im_out = im_in, re_in, im_out, re_out
    if kind == "real" and sw["real_packed"] and (L == 13 or (L == 14 and batch >= 8)) and _a(16, re_in):
        return {"fft_real_kernel"}
    if L - MAX_LOG2N > MAX_LOG2N1:
        return {"bigfft", "bigfft-scratch4" if aliased else "bigfft-out-scratch"} | _bigfft_rows(L, sw)
    if L > MAX_LOG2N:
        return {"fourstep-fused"}
    planes32 = _a(32, re_in, im_in, re_out, im_out)
    if 1 <= L <= 4 and sw["staged_small"] and planes32:
        return {"fft_tiny_staged_kernel"}
    if 5 <= L <= 7 and sw["staged_small"] and planes32:
        return {"fft_staged_kernel"}
    if L == 13 and kind != "real" and sw["split16k"] and _a(16, re_in, im_in):
        return {"fft_split2_kernel"}
    return {"fft_stockham_kernel"}


def _peak_names(bins, outputs):
    if "idx" not in outputs:
        return set()
    return {"peak_wave_kernel" if bins <= 2048 else "find_peak_kernel"}


def _spectrum_path(L, batch, offs, frame_len, stride, window, sides, outputs, sw):
    n = 1 << L
    f_off, w_off = offs
    used = min(frame_len, n)
    bins = n // 2 + 1 if sides == "one" else n
    if used == 0:
        return {"memset"}
    if 6 <= L <= 14:  # the packed-real tables (an N/2-point transform) exist up to N = 2^14
        fast = _a(16, f_off, w_off) and stride % 2 == 0 and used == n and sides == "one" and "ph" not in outputs
        wmode = 1 if window else 0  # f64: a plan's rect window is read as a table of ones
        return {f"spectrum_packed_kernel-{'FAST' if fast else 'general'}-m{L - 1}-w{wmode}"} | \
            _peak_names(bins, outputs)
    if L > MAX_LOG2N:
        if L - MAX_LOG2N > MAX_LOG2N1:
            return {"bigfft_out<AMP>"} | _bigfft_rows(L, sw) | _peak_names(bins, outputs)
        return {"fourstep_out_kernel<AMP>"} | _peak_names(bins, outputs)
    if 1 <= L <= 5 and sw["staged_small"] and used == n and stride == n and "ph" not in outputs and _a(32, f_off):
        return {"fft_tiny_staged_kernel<AMP>"} | _peak_names(bins, outputs)
    return {"small-complex-(x,0)"} | _peak_names(bins, outputs)


REQUIRED_F64 = {
    # transforms
    "fft_tiny_staged_kernel", "fft_staged_kernel", "fft_stockham_kernel", "fft_split2_kernel", "fft_real_kernel",
    "fourstep-fused", "bigfft", "bigfft-n1-staged", "bigfft-n1-stockham-tw1", "bigfft-n1-split2", "bigfft-scratch4",
    "bigfft-out-scratch",
    # spectra
    "fft_tiny_staged_kernel<AMP>", "small-complex-(x,0)",
    *[f"spectrum_packed_kernel-{f}-m{m}-w{w}" for f in ("FAST", "general") for m in range(5, 14) for w in (0, 1)],
    "fourstep_out_kernel<AMP>", "bigfft_out<AMP>", "peak_wave_kernel", "find_peak_kernel", "memset",
}


# ---- the dispatch, asked ----------------------------------------------------------------------------------------

def path_names_f64(info, n, spectrum=False):
    """expected_path_f64()'s names for the decision the library reports in `info` (include/pdsp_hip_dev.h)."""
    (path, rows, n1_rows, n1_square, np_, t0, t1, t2, tile_major, pairs, out_first, fast, wmode, first, fused_peaks,
     peaks, head) = info
    L = n.bit_length() - 1
    assert np_ == 0 and not fused_peaks and path not in (5, 7, 8, 12, 13, 14), list(info)  # the f32-only forms
    peak = {name for bit, name in PEAK_NAME.items() if peaks & bit}
    bigrows = set()
    if path == 10:
        form = "bigfft-n1-split2" if n1_square else {2: "bigfft-n1-staged", 3: "bigfft-n1-stockham-tw1"}[n1_rows]
        bigrows = {form, ROWS_NAME[n1_rows], ROWS_NAME[rows]}
    if not spectrum:
        assert peak == set(), list(info)
        if path == 10:
            assert pairs == (1 if out_first else 2), list(info)
            return {"bigfft", "bigfft-out-scratch" if out_first else "bigfft-scratch4"} | bigrows
        return {{1: "fft_tiny_staged_kernel", 2: "fft_staged_kernel", 3: "fft_stockham_kernel", 4: "fft_split2_kernel",
                 6: "fft_real_kernel", 9: "fourstep-fused"}[path]}
    if path == 15:
        return {f"spectrum_packed_kernel-{'FAST' if fast else 'general'}-m{L - 1}-w{wmode}"} | peak
    if path == 10:
        return {"bigfft_out<AMP>"} | bigrows | peak
    return {{9: "fourstep_out_kernel<AMP>", 11: "memset", 16: "fft_tiny_staged_kernel<AMP>",
             17: "small-complex-(x,0)"}[path]} | peak


def asked_path(fn, n, *args, spectrum=False):
    """The names for what the query `fn` reports for a call with these arguments."""
    import ctypes
    info = (ctypes.c_int * PATH_INFO)(*([-1] * PATH_INFO))
    assert fn(*args, info) == 0, _lib().pdsp_last_error()
    return path_names_f64(list(info), n, spectrum)


# ---- extended-precision references ------------------------------------------------------------------------------

def check_long_double():
    """numpy computes FFTs of np.longdouble in the x87 80-bit format here, or this file has no reference."""
    eps = float(np.finfo(np.longdouble).eps)
    assert eps < 1e-18, f"np.longdouble eps {eps}: no extended precision on this host"
    z = np.fft.fft(np.ones(4, dtype=np.longdouble))
    assert z.dtype == np.clongdouble and z.dtype.itemsize == 32, z.dtype


def _ld(a):
    return np.asarray(a).astype(np.longdouble)


def ld_fft(z, inverse=False, real=False):
    """fft / ifft / rfft over the last axis in long double; asserts the complex256 result."""
    if real:
        out = np.fft.rfft(z, axis=-1)
    else:
        out = np.fft.ifft(z, axis=-1) if inverse else np.fft.fft(z, axis=-1)
    assert out.dtype == np.clongdouble and out.dtype.itemsize == 32, out.dtype
    return out


def reference_transform(kind, re, im):
    z = _ld(re) if im is None else _ld(re) + 1j * _ld(im)
    return ld_fft(z, inverse=kind in ("inverse", "iinv"))


def split(ref):
    """(hi, lo) f64 parts of a long-double array: hi + lo == ref to ~2^-106."""
    hi = ref.astype(np.complex128 if np.iscomplexobj(ref) else np.float64)
    lo = (ref - hi).astype(hi.dtype)
    return hi, lo


def row_errors(got, ref, floor=None):
    """The f32 file's metric against a long-double reference: max_k |got_k - ref_k| / scale_k per row, the difference
    taken as (got - hi) - lo; rows whose reference is all zeros must be exactly zero (error 0 or inf)."""
    hi, lo = split(np.asarray(ref))
    den = scale(hi, floor)
    d = np.abs((np.asarray(got) - hi) - lo)
    r = np.where(den > 0, d / np.where(den > 0, den, 1.0), np.where(d == 0, 0.0, np.inf))
    return np.where(np.isnan(d), np.inf, r).max(axis=-1)


# ---- buffers and calls ------------------------------------------------------------------------------------------

def _lib():
    from pragma_dsp_amd._capi import lib
    return lib


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def dbuf(rows, length, off=0, stride=None, fill=float("nan")):
    import torch
    return Buf(rows, length, off, stride, fill, dtype=torch.float64)


_PLANS = {}


def plan(n):
    import torch
    from pragma_dsp_amd.batch import BatchedFft
    if n not in _PLANS:
        _PLANS[n] = BatchedFft(n, "cuda:0", dtype=torch.float64)
    return _PLANS[n]


def drop_plan(n):
    import torch
    p = _PLANS.pop(n, None)
    if p is not None:
        p.close()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def _release_plans():
    import torch
    check_long_double()
    yield
    for p in _PLANS.values():
        p.close()
    _PLANS.clear()
    torch.cuda.empty_cache()


ROW_KINDS = ("gauss", "peaky", "impulse", "const", "zero")


def make_rows(rng, batch, n, complex_, kinds=None, first=0):
    """The f32 file's rows without the f32 rounding: (re, im or None) in f64."""
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
    return re, im


def run_transform(kind, n, re, im, offs, out_mode="disjoint", switches=None):
    """One raw f64 transform call with planes at `offs` doubles (re_in, im_in, re_out, im_out) inside NaN-guarded
    buffers.  out_mode: disjoint, inplace (out planes = in planes), overlap (re_out starts half a plane plus offs[2]
    doubles into re_in's buffer).  Returns (got complex, path names)."""
    import torch
    batch = re.shape[0]
    lib, p = _lib(), plan(n)
    if kind in ("ifwd", "iinv"):
        zin = dbuf(batch, 2 * n, offs[0])
        z = np.empty((batch, 2 * n))
        z[:, 0::2], z[:, 1::2] = re, im
        zin.set(z)
        zout = dbuf(batch, 2 * n, offs[2])
        fn = lib.pdsp_fft_inverse_interleaved_f64 if kind == "iinv" else lib.pdsp_fft_forward_interleaved_f64
        with Switches(switches):
            assert fn(p._h, batch, zin.ptr, zout.ptr, _stream()) == 0, lib.pdsp_last_error()
        torch.cuda.synchronize()
        assert zin.outside_ok() and zout.outside_ok(), "write outside the rows"
        g = zout.get()
        return g[:, 0::2] + 1j * g[:, 1::2], expected_path_f64(kind, n, batch, offs, switches=switches)
    bre = dbuf(batch, n, offs[0])
    bre.set(re)
    bim = None
    if kind != "real":
        bim = dbuf(batch, n, offs[1])
        bim.set(im)
    im_ptr = bim.ptr if bim is not None else None
    im_off = offs[1] if kind != "real" else None
    if out_mode == "inplace":
        oim = bim if bim is not None else dbuf(batch, n, offs[3])
        ore_ptr, read_re = bre.ptr, bre.get
        poffs = (offs[0], im_off, offs[0], offs[1] if kind != "real" else offs[3])
        checks = [bre, oim]
    elif out_mode == "overlap":
        shift = (batch * n) // 2 + offs[2]
        big = dbuf(1, batch * n + shift, offs[0])
        big.flat[big.start:big.start + batch * n].copy_(bre.view.reshape(-1))
        bre = big
        oim = dbuf(batch, n, offs[3])
        ore_ptr = big.ptr + 8 * shift
        read_re = lambda: big.get()[0, shift:].reshape(batch, n)  # noqa: E731
        poffs = (offs[0], im_off, offs[0] + shift, offs[3])
        checks = [big, oim]
    else:
        ore, oim = dbuf(batch, n, offs[2]), dbuf(batch, n, offs[3])
        ore_ptr, read_re = ore.ptr, ore.get
        poffs = (offs[0], im_off, offs[2], offs[3])
        checks = [ore, oim]
    s = _stream()
    mirror = expected_path_f64(kind, n, batch, poffs, aliasing=out_mode != "disjoint", switches=switches)
    with Switches(switches):
        path = asked_path(lib.pdsp_dev_transform_path_f64, n, p._h, batch, bre.ptr, im_ptr, ore_ptr, oim.ptr,
                          1 if kind == "inverse" else 0)
        assert path == mirror, (kind, n, batch, poffs, out_mode, switches, sorted(path), sorted(mirror))
        if kind == "complex":
            rc = lib.pdsp_fft_forward_complex_f64(p._h, batch, bre.ptr, im_ptr, ore_ptr, oim.ptr, s)
        elif kind == "real":
            rc = lib.pdsp_fft_forward_real_f64(p._h, batch, bre.ptr, ore_ptr, oim.ptr, s)
        else:
            rc = lib.pdsp_fft_inverse_f64(p._h, batch, bre.ptr, im_ptr, ore_ptr, oim.ptr, s)
        torch.cuda.synchronize()
    assert rc == 0, lib.pdsp_last_error()
    for b in checks:
        assert b.outside_ok(), "write outside the output planes"
    got = read_re() + 1j * oim.get()
    return got, path


def _tf_kind(kind):
    return "inv" if kind in ("inverse", "iinv") else "fwd"


def check_transform(worst, kind, n, got, ref, ctx):
    errs = row_errors(got, ref)
    e = worst.add(_tf_kind(kind), n, errs)
    zero = np.all(ref == 0, axis=-1)
    if zero.any():
        assert (got[zero] == 0).all(), (ctx, "zero row not exactly zero")
    return [(ctx, e / lg(n))] if e > bound(_tf_kind(kind), n) else []


# (id, log2 sizes, batch, kinds, plane offsets re_in / im_in / re_out / im_out in doubles, out mode, switches,
#  intended names)
T = ("complex", "real", "inverse")
TRANSFORM_CASES = [
    ("tiny-32B", range(1, 5), 37, T, (0, 4, 8, 12), "disjoint", None, {"fft_tiny_staged_kernel"}),
    ("stockham-n1", range(0, 1), 9, T, (1, 3, 2, 0), "disjoint", None, {"fft_stockham_kernel"}),
    ("stockham-small-off1", range(1, 8), 7, T, (1, 0, 0, 0), "disjoint", None, {"fft_stockham_kernel"}),
    ("stockham-small-off2", range(1, 8), 5, T, (0, 0, 2, 0), "disjoint", None, {"fft_stockham_kernel"}),
    ("stockham-staged-off", range(1, 8), 33, T, (0, 0, 0, 0), "disjoint", {"staged_small": 0}, {"fft_stockham_kernel"}),
    ("staged", range(5, 8), 33, T, (4, 0, 0, 4), "disjoint", None, {"fft_staged_kernel"}),
    ("stockham-256-4096", range(8, 13), 5, T, (0, 0, 0, 0), "disjoint", None, {"fft_stockham_kernel"}),
    ("interleaved", range(0, 14), 3, ("ifwd", "iinv"), (2, 0, 6, 0), "disjoint", None, {"fft_stockham_kernel"}),
    # launch_rows decides aligned16 from the input planes only: 16-byte inputs, outputs off by 1 / 3 doubles
    ("split2", range(13, 14), 3, ("complex", "inverse"), (2, 4, 1, 3), "disjoint", None, {"fft_split2_kernel"}),
    ("stockham-8192-in-off", range(13, 14), 3, ("complex", "inverse"), (1, 0, 0, 0), "disjoint", None,
     {"fft_stockham_kernel"}),
    ("stockham-8192-split0", range(13, 14), 2, ("complex", "inverse"), (0, 0, 0, 0), "disjoint", {"split16k": 0},
     {"fft_stockham_kernel"}),
    ("real-8192", range(13, 14), 3, ("real",), (2, 0, 1, 3), "disjoint", None, {"fft_real_kernel"}),
    ("real-8192-in-off", range(13, 14), 3, ("real",), (1, 0, 0, 0), "disjoint", None, {"fft_stockham_kernel"}),
    ("real-8192-packed0", range(13, 14), 3, ("real",), (0, 0, 0, 0), "disjoint", {"real_packed": 0},
     {"fft_stockham_kernel"}),
    ("real-16384-b8", range(14, 15), 8, ("real",), (0, 0, 3, 1), "disjoint", None, {"fft_real_kernel"}),
    ("real-16384-b8-packed0", range(14, 15), 8, ("real",), (0, 0, 0, 0), "disjoint", {"real_packed": 0},
     {"fourstep-fused"}),
    ("fourstep", range(14, 18), 2, T, (0, 0, 0, 0), "disjoint", None, {"fourstep-fused"}),
    ("fourstep-unaligned", range(14, 18), 2, T, (1, 3, 2, 1), "disjoint", None, {"fourstep-fused"}),
    ("fourstep-inplace", range(14, 16), 2, ("complex", "inverse"), (0, 4, 0, 0), "inplace", None, {"fourstep-fused"}),
    ("bigfft-staged", range(18, 21), 2, T, (0, 0, 0, 0), "disjoint", None, {"bigfft-n1-staged"}),
    ("bigfft-staged-off", range(18, 19), 1, ("complex", "inverse"), (0, 0, 0, 0), "disjoint", {"staged_small": 0},
     {"bigfft-n1-stockham-tw1"}),
    ("bigfft-tw1", range(21, 22), 1, T, (0, 0, 0, 0), "disjoint", None, {"bigfft-n1-stockham-tw1"}),
    ("bigfft-unaligned", range(19, 22), 1, T, (1, 3, 2, 1), "disjoint", None, {"bigfft"}),
    ("bigfft-inplace", range(18, 22, 3), 2, ("complex", "real", "inverse"), (0, 4, 0, 6), "inplace", None,
     {"bigfft-scratch4"}),
    ("bigfft-overlap", range(18, 20), 2, ("complex", "real", "inverse"), (0, 4, 4, 0), "overlap", None,
     {"bigfft-scratch4"}),
]


@pytest.mark.parametrize("case", TRANSFORM_CASES, ids=[c[0] for c in TRANSFORM_CASES])
def test_transform_paths(record_property, case):
    name, logs, batch, kinds, offs, out_mode, sw, intended = case
    rng = np.random.default_rng(sum(map(ord, name)))
    worst = Worst(record_property, name)
    fails = []
    for L in logs:
        n = 1 << L
        for i, kind in enumerate(kinds):
            re, im = make_rows(rng, batch, n, kind != "real", first=L + i)
            got, path = run_transform(kind, n, re, im, offs, out_mode, sw)
            assert intended <= path, (name, L, kind, sorted(path))
            fails += check_transform(worst, kind, n, got, reference_transform(kind, re, im), (name, L, kind))
    worst.record()
    assert not fails, fails


# ---- the top of the range ---------------------------------------------------------------------------------------
# One row per call.  The bigfft N1 pass: stockham with tw1 at 2^21 ... 2^25, launch_rows (fft_split2_kernel) at 2^26.
TOP_N = [1 << 22, 1 << 23, 1 << 24, 1 << 25, 1 << 26]
TOP_MODES = (("aligned", (0, 0, 0, 0), "disjoint"), ("misaligned", (1, 3, 2, 1), "disjoint"),
             ("inplace", (0, 0, 0, 0), "inplace"))


def _mem_available():
    with open("/proc/meminfo") as f:
        for line in f:
            if line.startswith("MemAvailable:"):
                return int(line.split()[1]) * 1024
    return 0


@pytest.mark.parametrize("n", TOP_N, ids=[f"2p{n.bit_length() - 1}" for n in TOP_N])
def test_top_of_range_transforms(record_property, n):
    """f64 complex, real and inverse transforms at 2^22 ... 2^26: aligned, misaligned and in place, one reference per
    kind; at 2^26 also the host drop-in (Radix2Fft in f64 mode) on the same rows."""
    # a long-double row of 2^26 points is 1 GiB; the reference and the comparison hold about eight such arrays
    assert _mem_available() >= 12 * 16 * n, "host memory for the long-double reference"
    L = n.bit_length() - 1
    rng = np.random.default_rng(L)
    worst = Worst(record_property, f"top{L}")
    fails = []
    for i, kind in enumerate(T):
        re, im = make_rows(rng, 1, n, kind != "real", kinds=("gauss", "peaky", "impulse"), first=L + i)
        ref = reference_transform(kind, re, im)
        for mode, offs, out_mode in TOP_MODES:
            got, path = run_transform(kind, n, re, im, offs, out_mode)
            want = "bigfft-n1-split2" if L == 26 else "bigfft-n1-stockham-tw1"
            assert want in path and "bigfft" in path, (L, kind, mode, sorted(path))
            fails += check_transform(worst, kind, n, got, ref, (L, kind, mode))
            del got
        if L == 26:
            import pragma_dsp_amd as pd
            lib = _lib()
            prev = lib.pdsp_set_host_precision(64)
            try:
                fft = pd.Radix2Fft(n)
                if kind == "real":
                    out = fft.forward(re[0])
                elif kind == "complex":
                    out = fft.forwardComplex(pd.ComplexArray(re[0].copy(), im[0].copy()))
                else:
                    out = fft.inverse(pd.ComplexArray(re[0].copy(), im[0].copy()))
                got = (np.asarray(out.real) + 1j * np.asarray(out.imag))[None]
                del fft, out
            finally:
                lib.pdsp_set_host_precision(prev)
            fails += check_transform(worst, kind, n, got, ref, (L, kind, "drop-in"))
            del got
        del ref
    drop_plan(n)
    worst.record()
    assert not fails, fails


# ---- spectra ----------------------------------------------------------------------------------------------------

def copy_plan_window(n, kind, dst_ptr):
    """Copy the plan's device table (pdsp_plan_window_f64, the window every f64 kernel reads) to `dst_ptr`, bit for
    bit: pdsp_apply_window_f64 on a row of ones."""
    import torch
    lib = _lib()
    ones = torch.ones(n, dtype=torch.float64, device="cuda:0")
    rc = lib.pdsp_apply_window_f64(1, n, ones.data_ptr(), plan(n).window(kind).data_ptr(), dst_ptr, _stream())
    assert rc == 0, lib.pdsp_last_error()
    torch.cuda.synchronize()


def plan_window(n, kind):
    """The plan's f64 device table, on the host."""
    import torch
    w = torch.empty(n, dtype=torch.float64, device="cuda:0")
    copy_plan_window(n, kind, w.data_ptr())
    return w.cpu().numpy()


def reference_spectrum(frames, n, win, sides):
    """(amplitude, X over the bins returned, scale per bin): spectrum()'s body in long double."""
    x = np.zeros((frames.shape[0], n), dtype=np.longdouble)
    m = min(frames.shape[1], n)
    x[:, :m] = frames[:, :m]
    if win is not None:
        x = x * _ld(win)
    if sides == "one":
        X = ld_fft(x, real=True)
        sc = np.full(n // 2 + 1, 2.0 / n)
        sc[0] = 1.0 / n
        if n % 2 == 0:
            sc[n // 2] = 1.0 / n
    else:
        X = ld_fft(x)
        sc = np.full(n, 1.0 / n)
    return np.abs(X) * _ld(sc), X, sc


def run_spectrum(n, rows, frame_len, stride, f_off, window, w_off, sides, outputs, switches=None, signal=None):
    """One raw pdsp_spectrum_f64 call.  rows: [batch, min(frame_len, N)] placed at `stride` in a NaN buffer (or
    `signal` for overlapping frames); samples past min(frame_len, N) of each row are NaN, so reading them shows.
    window: None, ("plan", kind) or ("table", kind) (a copy of the plan's table at w_off doubles).  Returns dict of
    outputs + path."""
    import torch
    lib, p = _lib(), plan(n)
    batch = rows.shape[0]
    used = min(frame_len, n)
    if signal is not None:
        fb = dbuf(1, signal.size, f_off)
        fb.set(signal[None])
    else:
        fb = dbuf(batch, max(frame_len, 1), f_off, stride=stride) if batch else dbuf(1, 1, f_off)
        full = np.full((batch, max(frame_len, 1)), np.nan)
        full[:, :used] = rows[:, :used]
        fb.set(full)
    wptr, wb = None, None
    if window is not None and window[0] == "plan":
        wptr = p.window(window[1]).data_ptr()
        w_off = 0
    elif window is not None:
        wb = dbuf(1, n, w_off)
        copy_plan_window(n, window[1], wb.ptr)
        wptr = wb.ptr
    bins = n // 2 + 1 if sides == "one" else n
    out = {}
    amp = dbuf(batch, bins) if "amp" in outputs else None
    ph = dbuf(batch, bins, 1) if "ph" in outputs else None
    idx = Buf(batch, 1, 0, fill=SENT_I32, dtype=torch.int32) if "idx" in outputs else None
    ptr = lambda b: b.ptr if b is not None else None  # noqa: E731
    mirror = expected_path_f64("spectrum", n, batch, (f_off, w_off if window else None), frame_len=frame_len,
                               stride=stride, window=window, sides=sides, outputs=outputs, switches=switches)
    with Switches(switches):
        path = asked_path(lib.pdsp_dev_spectrum_path_f64, n, p._h, batch, fb.ptr, frame_len, stride, wptr,
                          1 if sides == "two" else 0, ptr(amp), ptr(ph), ptr(idx), None, 1.0, spectrum=True)
        assert path == mirror, (n, batch, frame_len, stride, f_off, window, w_off, sides, sorted(outputs), switches,
                                sorted(path), sorted(mirror))
        rc = lib.pdsp_spectrum_f64(p._h, batch, fb.ptr, frame_len, stride, wptr, 1 if sides == "two" else 0, ptr(amp),
                                   ptr(ph), ptr(idx), _stream())
        torch.cuda.synchronize()
    assert rc == 0, lib.pdsp_last_error()
    assert fb.outside_ok() and (wb is None or wb.outside_ok()), "write to an input"
    for k, b in (("amp", amp), ("ph", ph), ("idx", idx)):
        if b is not None:
            assert b.outside_ok(), f"{k}: write outside the output rows"
            out[k] = b.get()
    out["path"] = path
    return out


def check_spectrum(worst, n, frames, out, window, sides, ctx):
    """Amplitude, phase and peak index of one call against the long-double reference; returns the failures."""
    win = plan_window(n, window[1]) if window else None
    amp_ref, X, sc = reference_spectrum(frames, n, win, sides)
    b_amp = bound("amp", n)
    fails = []
    amp_hi = amp_ref.astype(np.float64)
    rms = np.sqrt((amp_hi ** 2).mean(axis=-1))
    zero = rms == 0
    den = scale(amp_hi)
    zero_in = (frames == 0).all(axis=-1)
    if "amp" in out:
        a = out["amp"]
        assert not np.isnan(a).any(), (ctx, "NaN left in amplitude rows")
        e = worst.add("amp", n, row_errors(a, amp_ref))
        if e > b_amp:
            fails.append((ctx, "amp", e / lg(n)))
        if zero.any():
            assert (a[zero] == 0).all(), ctx
    if "ph" in out:
        ph = out["ph"]
        assert not np.isnan(ph).any(), (ctx, "NaN left in phase rows")
        mag = np.abs(X).astype(np.float64) * sc
        ok = (mag >= 1e-3 * rms[:, None]) & ~zero[:, None]
        d = np.abs(np.remainder(_ld(ph) - np.angle(X) + np.pi, 2 * np.pi) - np.pi).astype(np.float64)
        lim = PHASE_C * b_amp * den / np.where(ok, mag, 1.0)
        lim_max = float(lim[ok].max(initial=0))
        worst.w["phase_limit"] = max(worst.w.get("phase_limit", 0.0), lim_max)
        if n <= OLD_PHASE_MAX_N and lim_max >= OLD_PHASE_TOL:
            fails.append((ctx, "phase bound not tighter than 1e-9 rad", lim_max))
        if (d[ok] > lim[ok]).any():
            fails.append((ctx, "phase", float((d / lim)[ok].max())))
        worst.w["phase_in_bound"] = max(worst.w.get("phase_in_bound", 0.0), float((d / lim)[ok].max(initial=0)))
        if zero_in.any():
            assert (ph[zero_in] == 0).all(), (ctx, "phase of an all-zero row")
    if "idx" in out:
        got = out["idx"][:, 0].astype(np.int64)
        for r in range(frames.shape[0]):
            g = int(got[r])
            A = amp_hi[r]
            cand = A[1:]
            if zero[r] or cand.max(initial=0) <= 0:
                assert g == 0, (ctx, "idx", r, g)
                continue
            kr = 1 + int(np.argmax(cand))
            tie = 0 < g < A.size and A[g] >= A[kr] - 2 * b_amp * den[r, kr]
            mirror = sides == "two" and g == n - kr
            assert g == kr or mirror or tie, (ctx, "idx", r, g, kr)
    return fails


# (id, log2 sizes, batch, frame mode, stride mode, frames offset, windows, window offset, sides, output sets,
#  switches, intended name prefixes)
#   frame mode: full (N), part (about 2N/3), long (N + 5), zero (0); stride mode: len (= frame length), gap<k>
#   (frame length + k), hop<k> (overlapping frames N/k apart)
A, P, I = ("amp",), ("amp", "ph"), ("amp", "idx")
W_ALL = (None, ("plan", "rect"), ("plan", "hann"), ("table", "hamming"))
SPEC_CASES = [
    ("tiny-amp", range(1, 6), 37, "full", "len", 0, W_ALL, 0, ("one", "two"), (A, I), None,
     ("fft_tiny_staged_kernel<AMP>",)),
    ("small-x0-n1", range(0, 1), 9, "full", "len", 1, (None,), 0, ("one", "two"), (A, P, I), None, ("small-complex",)),
    ("small-x0", range(1, 6), 11, "full", "len", 0, W_ALL, 0, ("one", "two"), (P,), None, ("small-complex",)),
    ("small-x0-off", range(1, 6), 5, "full", "len", 2, (None,), 0, ("one",), (A, I), None, ("small-complex",)),
    ("small-x0-part", range(1, 6), 5, "part", "gap3", 1, (None, ("table", "hann")), 1, ("one",), (A, I), None,
     ("small-complex",)),
    ("small-x0-hop", range(2, 6), 6, "full", "hop2", 2, (("plan", "hann"),), 0, ("two",), (P,), None,
     ("small-complex",)),
    ("small-x0-long", range(1, 6), 4, "long", "len", 0, (None,), 0, ("one",), (A,), None, ("small-complex",)),
    ("tiny-off", range(1, 6), 5, "full", "len", 0, (None,), 0, ("one",), (A,), {"staged_small": 0},
     ("small-complex",)),
    ("packed-fast", range(6, 15), 5, "full", "len", 0, (None, ("table", "hann"), ("plan", "rect")), 0, ("one",),
     (A, I), None, ("spectrum_packed_kernel-FAST",)),
    ("packed-fast-stride", range(6, 15), 3, "full", "gap2", 2, (None, ("plan", "hann")), 0, ("one",), (A,), None,
     ("spectrum_packed_kernel-FAST",)),
    ("packed-general-phase", range(6, 15), 3, "full", "len", 0, (None, ("table", "blackman")), 0, ("one",), (P,),
     None, ("spectrum_packed_kernel-general",)),
    ("packed-general-two", range(6, 15), 3, "full", "len", 0, (None, ("plan", "hamming")), 0, ("two",), (A, I), None,
     ("spectrum_packed_kernel-general",)),
    ("packed-general-part", range(6, 15), 3, "part", "gap1", 1, (("table", "hann"),), 1, ("one",), (A, I), None,
     ("spectrum_packed_kernel-general",)),
    ("packed-general-long", range(6, 12), 3, "long", "len", 0, (None,), 0, ("one",), (A,), None,
     ("spectrum_packed_kernel-general",)),
    ("packed-hop", range(6, 15), 5, "full", "hop4", 0, (("plan", "hann"),), 0, ("one",), (A,), None,
     ("spectrum_packed_kernel-FAST",)),
    # the FAST predicate with a window table at an odd double offset
    ("packed-win-odd", range(6, 15), 3, "full", "len", 0, (("table", "hann"),), 1, ("one",), (A,), None,
     ("spectrum_packed_kernel-general",)),
    ("fourstep-spec", range(15, 18), 2, "full", "len", 0, W_ALL, 0, ("one", "two"), (A, P, I), None,
     ("fourstep_out_kernel<AMP>",)),
    ("fourstep-spec-part", range(15, 18), 2, "part", "gap2", 1, (None, ("plan", "hann")), 0, ("one",), (A, I), None,
     ("fourstep_out_kernel<AMP>",)),
    ("bigfft-spec", range(18, 22), 1, "full", "len", 0, (("plan", "hann"),), 0, ("one",), (A, I), None,
     ("bigfft_out<AMP>",)),
    ("bigfft-spec-part", range(18, 20), 2, "part", "gap1", 1, (None, ("table", "blackman")), 3, ("one", "two"), (P,),
     None, ("bigfft_out<AMP>",)),
    ("bigfft-spec-staged-off", range(18, 19), 1, "long", "len", 0, (None,), 0, ("one",), (A,), {"staged_small": 0},
     ("bigfft-n1-stockham-tw1",)),
    ("memset", range(0, 15, 7), 3, "zero", "gap1", 0, (None,), 0, ("one", "two"), (P, I), None, ("memset",)),
]


def _frame_geometry(n, frame, stride_mode):
    length = {"full": n, "part": max(n - n // 3 - 1, 1), "long": n + 5, "zero": 0}[frame]
    if stride_mode == "len":
        return length, max(length, 1), None
    if stride_mode.startswith("gap"):
        return length, max(length, 1) + int(stride_mode[3:]), None
    return length, max(n // int(stride_mode[3:]), 1), "hop"


def spectrum_rows(rng, batch, n, length, stride, hop, first):
    """(rows [batch, used] in f64, the signal for overlapping frames or None)."""
    used = min(length, n)
    if hop:
        sig = rng.standard_normal((batch - 1) * stride + used)
        sig[: used // 2] += 3 * np.cos(2 * np.pi * 0.21 * np.arange(used // 2))
        rows = np.stack([sig[b * stride:b * stride + used] for b in range(batch)])
        return rows, sig
    re, _ = make_rows(rng, batch, max(used, 1), False, first=first)
    return re[:, :used], None


@pytest.mark.parametrize("case", SPEC_CASES, ids=[c[0] for c in SPEC_CASES])
def test_spectrum_paths(record_property, case):
    name, logs, batch, frame, smode, f_off, windows, w_off, sidess, outsets, sw, want = case
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
                    assert any(p.startswith(w) for p in out["path"] for w in want), ctx
                    if length == 0:
                        for k in ("amp", "ph", "idx"):
                            if k in out:
                                assert (out[k] == 0).all(), ctx
                        continue
                    fails += check_spectrum(worst, n, rows, out, window, sides, ctx)
    worst.record()
    assert not fails, fails


TOP_SPEC_N = [1 << 22, 1 << 23, 1 << 24, 1 << 25, 1 << 26]


@pytest.mark.parametrize("n", TOP_SPEC_N, ids=[f"2p{n.bit_length() - 1}" for n in TOP_SPEC_N])
def test_top_of_range_spectra(record_property, n):
    """One Hann-windowed frame at 2^22 ... 2^26 through bigfft AMP (launch_rows N1 pass at 2^26), amplitude, phase and
    peak index, and an unaligned frame of N + 5 samples (the general loader)."""
    L = n.bit_length() - 1
    rng = np.random.default_rng(200 + L)
    worst = Worst(record_property, f"topspec{L}")
    fails = []
    rows, _ = make_rows(rng, 1, n + 5, False, kinds=("peaky", "gauss"), first=L)
    want = "bigfft-n1-split2" if L == 26 else "bigfft-n1-stockham-tw1"
    for frame_len, f_off, outs in ((n, 0, ("amp", "idx")), (n + 5, 1, ("amp", "ph"))):
        out = run_spectrum(n, rows[:, :min(frame_len, n)], frame_len, frame_len, f_off, ("plan", "hann"), 0, "one",
                           set(outs))
        ctx = (L, frame_len, f_off, sorted(out["path"]))
        assert want in out["path"] and "bigfft_out<AMP>" in out["path"], ctx
        fails += check_spectrum(worst, n, rows[:, :n], out, ("plan", "hann"), "one", ctx)
        del out
    drop_plan(n)
    worst.record()
    assert not fails, fails


def test_plan_windows_match_the_long_double_cosine_sum():
    """The f64 tables every f64 spectrum kernel reads (pdsp_plan_window_f64), against createWindow's cosine sums
    evaluated in long double: within 8 * 2^-53 absolute (windows are at most 1).  The table is createWindow's f64
    formula, whose argument 2 pi i / (N - 1) carries the rounding of pi: 3.4 * 2^-53 measured at N = 64, 6.3 * 2^-53
    (Blackman, N = 2^20) for the same formula on the host."""
    pi = np.arccos(np.longdouble(-1))
    for n in (2, 64, 1000 + 24, 1 << 14, 1 << 20):
        i = np.arange(n, dtype=np.longdouble)
        f = 2 * pi * i / (n - 1)
        want = {"rect": np.ones(n, dtype=np.longdouble), "hann": 0.5 * (1 - np.cos(f)),
                "hamming": np.longdouble("0.54") - np.longdouble("0.46") * np.cos(f),
                "blackman": np.longdouble("0.42") - 0.5 * np.cos(f) + np.longdouble("0.08") * np.cos(2 * f)}
        for kind, w in want.items():
            got = plan_window(n, kind)
            err = float(np.abs(_ld(got) - w).max())
            assert err <= 8 * 2.0 ** -53, (n, kind, err)
        drop_plan(n)


# ---- bitwise invariances ----------------------------------------------------------------------------------------

INV_T = [(3, 37, (0, 4, 8, 12)), (6, 33, (4, 0, 0, 4)), (7, 70, (1, 0, 0, 0)), (10, 9, (0, 0, 0, 0)),
         (13, 5, (2, 4, 0, 0)), (14, 3, (0, 0, 0, 0)), (16, 3, (1, 0, 0, 0)), (18, 3, (0, 0, 0, 0)),
         (21, 2, (0, 0, 0, 0))]
INV_S = [(4, 300, None, "one"), (5, 130, ("table", "hann"), "two"), (7, 200, None, "one"),
         (8, 33, ("plan", "hann"), "one"), (11, 9, ("plan", "blackman"), "one"), (12, 9, None, "two"),
         (14, 5, ("plan", "hann"), "one"), (15, 3, ("plan", "hamming"), "one"), (18, 3, None, "one"),
         (20, 2, ("plan", "hann"), "one")]


def _transform_once(n, re, im, offs, kind="complex"):
    got, _ = run_transform(kind, n, re, im, offs)
    return got


@pytest.mark.parametrize("L,batch,offs", INV_T, ids=[f"N{1 << c[0]}" for c in INV_T])
def test_transform_row_position_scaling_and_isolation(L, batch, offs):
    """A row gives the same bits alone and at several positions in a batch (the bigfft transposes move data between
    rows of a batch); scaling a row by 2^k scales its output bit for bit; NaN / Inf rows leave every other row's bits.
    Complex rows, and real rows where a real kernel exists (N = 8192, 16384 from 8 rows up)."""
    n = 1 << L
    rng = np.random.default_rng(L)
    kinds = ("complex", "real") if L in (13, 14) else ("complex",)
    for kind in kinds:
        b_ = batch if not (kind == "real" and L == 14) else 9
        re, im = make_rows(rng, b_, n, True, kinds=("gauss", "peaky", "impulse", "const"))
        im = im if kind == "complex" else None
        o = offs if kind == "complex" else (0, None, offs[2], offs[3])
        base = _transform_once(n, re, im, o, kind)
        # real rows of 16384 take fft_real_kernel from 8 rows up (four-step below): "alone" is then 8 rows
        m = 8 if (kind == "real" and L == 14) else 1
        for b in sorted({min(b, b_ - m) for b in (0, 1, b_ // 2, b_ - 1)}):
            alone = _transform_once(n, re[b:b + m], None if im is None else im[b:b + m], o, kind)
            assert np.array_equal(alone, base[b:b + m]), ("alone", n, kind, b)
        rolled = _transform_once(n, np.roll(re, 1, axis=0), None if im is None else np.roll(im, 1, axis=0), o, kind)
        assert np.array_equal(rolled, np.roll(base, 1, axis=0)), ("rolled", n, kind)
        for k in (-20, 17):
            sc = _transform_once(n, np.ldexp(re, k), None if im is None else np.ldexp(im, k), o, kind)
            want = np.ldexp(base.real, k) + 1j * np.ldexp(base.imag, k)
            assert np.array_equal(sc, want), ("scale", n, kind, k)
        bad_re = re.copy()
        bad_re[b_ // 2, n // 3] = np.nan
        bad_im = None
        if im is not None:
            bad_im = im.copy()
            if b_ > 2:
                bad_im[b_ - 1, n - 1] = np.inf
        elif b_ > 2:
            bad_re[b_ - 1, n - 1] = np.inf
        got = _transform_once(n, bad_re, bad_im, o, kind)
        keep = np.ones(b_, bool)
        keep[[b_ // 2, b_ - 1] if b_ > 2 else [b_ // 2]] = False
        assert np.array_equal(got[keep], base[keep]), ("isolation", n, kind)
        assert not np.isfinite(got[b_ // 2]).all()
    if L >= 18:
        drop_plan(n)


def _spectrum_once(n, rows, window, sides):
    return run_spectrum(n, rows, n, n, 0, window, 0, sides, {"amp"})["amp"]


@pytest.mark.parametrize("L,batch,window,sides", INV_S, ids=[f"N{1 << c[0]}" for c in INV_S])
def test_spectrum_row_position_scaling_and_isolation(L, batch, window, sides):
    """The same invariances for f64 amplitude rows: alone == in the batch, 2^k in == 2^k out, NaN / Inf isolated."""
    n = 1 << L
    rng = np.random.default_rng(100 + L)
    rows, _ = make_rows(rng, batch, n, False, kinds=("gauss", "peaky", "impulse", "const"))
    base = _spectrum_once(n, rows, window, sides)
    for b in sorted({0, 1, batch // 2, batch - 1}):
        assert np.array_equal(_spectrum_once(n, rows[b:b + 1], window, sides)[0], base[b]), ("alone", n, b)
    assert np.array_equal(_spectrum_once(n, np.roll(rows, 1, axis=0), window, sides), np.roll(base, 1, axis=0))
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
    if L >= 18:
        drop_plan(n)

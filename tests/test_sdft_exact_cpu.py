"""The exact fused multiply-add of sdft_ref (fma32 / fma64, in numpy) against libm's fmaf / fma, and the emulation of
the sliding DFT's summation order that is built on it (sdft_ref.emulate(exact=True), the form the device is held to bit
for bit in test_gpu_sdft_paths.py) against long double direct sums at the sizes where the kernel changes shape
(sdft_ref.PATH_SIZES).  No GPU.

The bound of the second part is sdft_ref.BOUND, unchanged.  Measured here (units of u sqrt(N) max|x|, worst over the
lengths, bins and rows of a size): 0.78 ... 2.44 in f32 and 0.001 (N = 2, all but exact) ... 1.94 in f64 against
8.92 / 8.84; the fma: 0 of 200 000 triples per precision differ from libm (the plain f64 product and sum: 116 376).
"""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

import sdft_ref as R

TRIPLES = 200_000


def triples(dtype, count, seed):
    """(a, b, c) of `count` values each in the precision `dtype`: Gaussian; the first half with c within a few ulp of
    -a b (the cancellation in which a second rounding shows); the last quarter scaled by 2^+-30 part by part."""
    rng = np.random.default_rng(seed)
    t = R.DT[dtype]
    a, b, c = (rng.standard_normal(count).astype(t) for _ in range(3))
    half, quarter = count // 2, count // 4
    ulps = rng.integers(-4, 5, half).astype(np.float64)
    near = -(a[:half].astype(np.float64) * b[:half].astype(np.float64)) * (1.0 + ulps * 2.0 * R.U[dtype])
    c[:half] = near.astype(t)
    for v in (a, b, c):
        v[-quarter:] *= (2.0 ** rng.choice([-30, 30], quarter)).astype(t)
    return a, b, c


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_exact_fma_is_libms(dtype):
    name = ctypes.util.find_library("m")
    assert name, "no libm"
    libm = C.CDLL(name)
    fn, ct, bits = (libm.fmaf, C.c_float, np.int32) if dtype == "f32" else (libm.fma, C.c_double, np.int64)
    fn.restype, fn.argtypes = ct, (ct, ct, ct)
    a, b, c = triples(dtype, TRIPLES, 2024)
    want = np.array([fn(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], dtype=R.DT[dtype])
    got = (R.fma32 if dtype == "f32" else R.fma64)(a, b, c)
    assert got.dtype == want.dtype and np.isfinite(want).all()
    bad = int((got.view(bits) != want.view(bits)).sum())
    # what the exact form is for: the product-and-sum it replaces (f32: in f64, rounded twice) against the same libm
    plain = a * b + c if dtype == "f64" else (a.astype(np.float64) * b + c.astype(np.float64)).astype(np.float32)
    loose = int((plain.view(bits) != want.view(bits)).sum())
    print(f"SDFT fma {dtype}: {bad} of {TRIPLES} triples differ from libm ({loose} for the product and sum)")
    assert bad == 0
    if dtype == "f64":
        assert loose > TRIPLES // 4  # the triples do tell the two apart


def test_exact_fma_broadcasts_and_keeps_shapes():
    # the emulation's calls: array x scalar weight + array, and 0-d operands
    for fma, t in ((R.fma32, np.float32), (R.fma64, np.float64)):
        a = np.arange(6, dtype=t).reshape(2, 3) / t(3)
        r = fma(a, t(0.25), a)
        assert r.shape == (2, 3) and r.dtype == t
        want = (a.astype(R.LD) * R.LD(0.25) + a.astype(R.LD)).astype(t)  # 64-bit significands: exact before rounding
        assert np.array_equal(r, want)
        assert fma(t(3), t(5), t(-15)) == 0 and fma(t(0), t(-1), t(0)) == 0


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("n,win", [(n, w) for n in R.PATH_SIZES for w in R.path_windows(n)])
def test_exact_emulation_against_direct_sums(n, win, dtype):
    """Every frame of the two rectangular bins 0 and 12.5 against one long double prefix sum, and the frames
    pick_frames names (all where they are few; the chunk and round boundaries else) against the definition, for every
    window, bin and row of the case."""
    rows, bins = R.path_shape(n, win)
    worst = worst_all = 0.0
    for t in R.path_lengths(n):
        x = R.signal(n, t)[:rows]
        xmax = np.abs(x).max()
        got = R.emulated(n, t, win, dtype, rows, bins)
        assert got.shape == (rows, len(bins), R.frames_of(n, 1, t))
        fr = R.pick_frames(n, 1, t)
        re, im = R.direct(x, n, bins, 1, win, fr)
        worst = max(worst, R.err_units(got[:, :, fr], re, im, n, dtype, xmax))
        if win == "rect":
            for j in (0, 1):
                sr, si = R.sliding(x, n, bins[j])
                worst_all = max(worst_all, R.err_units(got[:, j], sr, si, n, dtype, xmax))
    print(f"SDFT exact emulate {dtype} N={n} {win}: worst {worst:.3f} (all frames of two bins: {worst_all:.3f}) of the "
          f"bound {R.BOUND[dtype]:.2f} u sqrt(N) max|x|")
    assert worst <= R.BOUND[dtype] and worst_all <= R.BOUND[dtype]


def test_exact_and_plain_emulation_differ_only_in_the_fma():
    """The default form of emulate() is untouched by the keyword: f32 differs from the exact form in double roundings
    alone (a handful of values, each by one unit in the last place), f64 in most values."""
    n, t = 1025, 2 * 1025 + 1
    x = R.signal(n, t)[:1]
    for dtype, bits in (("f32", np.int32), ("f64", np.int64)):
        plain = R.emulate(x, n, (12.5,), 1, "hann", dtype)
        exact = R.emulate(x, n, (12.5,), 1, "hann", dtype, exact=True)
        p, e = (np.stack([v.real, v.imag]).view(bits) for v in (plain, exact))
        differ = int((p != e).sum())
        print(f"SDFT emulate {dtype} N={n} hann: {differ} of {p.size} values differ between the plain and the exact fma")
        assert differ <= p.size // 100 if dtype == "f32" else differ > p.size // 2
        assert np.abs(plain - exact).max() <= 64 * R.U[dtype] * np.sqrt(n) * np.abs(x).max()

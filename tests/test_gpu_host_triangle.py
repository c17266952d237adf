"""The promise of the batched host-f64 forms, as a triangle per size class: the chunked call == the one-shot sequence
(PDSP_HOST_THREADS=1) == the one-row calls, bit for bit -- pdsp_fft_transform_host_f64 / _rows_host_f64 and the three
batched spectrum forms against pdsp_spectrum_host_f64.  "Row b of the result is the one-shot result of row b" (above
kChunkInBytes in pdsp_capi_host.hip) and "Element i equals forward(inputs[i])" (core.py, js/core.js) hold only if the kernel
variant of a row never depends on how many rows travel with it, in the call or in a chunk of it.

The size classes come from the library: pdsp_dev_transform_path_f64 / _f32 over log2 N = 1 ... 18 / 19 for real, complex
and inverse calls of 1 and 64 rows; the smallest N of each distinct answer is a class, and the paths the classes reach
must cover REQUIRED, so a dispatch change fails here instead of dropping a class.  The classes are known only with a
device, after collection, so the cases are every power of two of that range -- a superset.  Batches are the smallest that
are cut into chunks plus a few rows, so that the last chunk is shorter than the others (TABLE holds the ones worked out by
hand); at N = 16384 also the batches around the device forms' 8-row threshold for f64 real rows (20 rows: every chunk
below it; 67: chunks of 8 and a tail of 3; 8 and 7 rows).

host_cut() mirrors chunk_in_bytes / host_workers / transform_cut / spectrum_cut of pdsp_capi_host.hip; every case asserts the
regime it names (chunked or not, rows per chunk, rows in the tail) on the mirror, and the mirror against the library's own
answer (pdsp_dev_host_transform_chunks / pdsp_dev_host_spectrum_chunks).  Every comparison of results is np.array_equal on
outputs pre-filled with NaN; the oracle is held on a few rows at the tolerances of test_gpu_host_chunked.py."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from test_gpu_host_chunked import capi, _peak_rows, _row_ptrs, _spectrum_batch, _transform  # noqa: F401  (capi: the fixture)

pytestmark = pytest.mark.gpu

PATH_INFO = 17
TINY, STAGED, STOCKHAM, SPLIT2, SPLIT4, REAL_PACKED, PAIRED, TILES, FOURSTEP, GENERAL = range(1, 11)
# tiny-staged, staged, Stockham, split2 / split4, real-packed, four-step and the general big path; and the two f32 forms
# beyond the single-pass limit
REQUIRED = {TINY, STAGED, STOCKHAM, SPLIT2, SPLIT4, REAL_PACKED, FOURSTEP, GENERAL, PAIRED, TILES}
MAX_LOG2 = {64: 18, 32: 19}
SINGLE_PASS_LOG2 = {64: 13, 32: 14}  # kMaxLog2N_f64 / _f32: above, transforms run on the multi-pass paths
THREADS = (2, 6)

# ---- the cut, restated (pdsp_capi_host.hip) ------------------------------------------------------------------------
CHUNK_IN_BYTES = 2 << 20
CHUNKED_MIN_BYTES = 4 << 20


def _workers(threads, multipass):
    v = threads
    if multipass and v > 2:
        v = 2
    return min(v, 16)


def _chunk_in_bytes(in_total, workers):
    return max(min(in_total // (2 * max(workers, 1)), CHUNK_IN_BYTES), 256 << 10)


def host_cut(kind, n, batch, precision, threads, bins=0):
    """(rows per chunk, workers, rows in the last chunk) of a host call under PDSP_HOST_THREADS=threads; (0, 0, 0): the
    one-shot sequence.  kind: transform / spectrum (bins = the rows' length out)."""
    e = precision // 8
    L = n.bit_length() - 1
    if kind == "transform":
        w = _workers(threads, L > SINGLE_PASS_LOG2[precision])
        per = _chunk_in_bytes(2 * batch * n * e, w) // (2 * n * e)
        big = 4 * batch * n * e >= CHUNKED_MIN_BYTES
    else:  # packed-real frames (N <= 16384) are one pass; above, the spectrum runs on multi-pass paths
        w = _workers(threads, L > 14)
        per = _chunk_in_bytes(batch * n * e, w) // (n * e)
        big = batch * (n + 2 * bins) * e >= CHUNKED_MIN_BYTES
    if not (w >= 2 and per >= 1 and batch >= 2 * per and big):
        return (0, 0, 0)
    nchunks = -(-batch // per)
    return (per, min(w, nchunks), batch - (nchunks - 1) * per)


def asked_cut(capi, kind, plan, batch, precision, threads, sides=0):
    os.environ["PDSP_HOST_THREADS"] = str(threads)
    info = (C.c_longlong * 2)(-1, -1)
    if kind == "transform":
        capi.check(capi.lib.pdsp_dev_host_transform_chunks(plan, batch, precision, info))
    else:
        capi.check(capi.lib.pdsp_dev_host_spectrum_chunks(plan, batch, sides, precision, info))
    return tuple(info)


def regime(capi, kind, plan, n, batch, precision, sides=0):
    """{threads: (per chunk, workers, tail)} from the mirror, checked against the library for THREADS and for 1."""
    bins = (n // 2 + 1 if sides == 0 else n) if kind == "spectrum" else 0
    assert asked_cut(capi, kind, plan, batch, precision, 1, sides) == (0, 0)
    cuts = {}
    for t in THREADS + (4,):
        cuts[t] = host_cut(kind, n, batch, precision, t, bins)
        assert asked_cut(capi, kind, plan, batch, precision, t, sides) == cuts[t][:2], (kind, n, batch, precision, t, cuts[t])
    return cuts


# ---- size classes from the library ----------------------------------------------------------------------------------

def _plan(capi, n):
    plan = C.c_void_p()
    capi.check(capi.lib.pdsp_plan_create(n, -1, C.byref(plan)))
    return plan


@functools.lru_cache(maxsize=None)
def size_classes(precision):
    """{N: set of paths} for the smallest N of each distinct dispatch answer (all PATH_INFO fields) over real, complex and
    inverse calls of 1 and 64 rows on planes aligned like staging (the queries only look at the addresses)."""
    import pragma_dsp_amd  # noqa: F401
    from pragma_dsp_amd import _capi
    q = _capi.lib.pdsp_dev_transform_path_f64 if precision == 64 else _capi.lib.pdsp_dev_transform_path_f32
    seen, out = set(), {}
    for L in range(1, MAX_LOG2[precision] + 1):
        n = 1 << L
        plan = _plan(_capi, n)
        try:
            for batch in (1, 64):
                base = [(1 + k) << 40 for k in range(4)]  # re_in, im_in, re_out, im_out: 4 KiB aligned, far apart
                for im_in, inverse in ((None, 0), (base[1], 0), (base[1], 1)):
                    info = (C.c_int * PATH_INFO)(*([-1] * PATH_INFO))
                    _capi.check(q(plan, batch, base[0], im_in, base[2], base[3], inverse, info))
                    key = (im_in is None, inverse, batch) + tuple(info)
                    if key not in seen:
                        seen.add(key)
                        out.setdefault(n, set()).add(info[0])
        finally:
            _capi.lib.pdsp_plan_destroy(plan)
    return out


# N -> batch: the smallest batch that is cut into chunks (4 MiB of staging) plus a few rows.  The largest size of each
# precision has rows too long for a chunk (2 x row > kChunkInBytes): never chunked, batch against one-row only.
TABLE = {
    64: {8: 16389, 64: 2053, 1024: 131, 8192: 19, 16384: 67, 32768: 9, 1 << 17: 5, 1 << 18: 3},
    32: {8: 32773, 64: 4101, 1024: 259, 8192: 37, 16384: 131, 32768: 17, 1 << 17: 9, 1 << 18: 5, 1 << 19: 3},
}
# the f64 regimes worked out by hand from the rule, as (N, batch, threads): (per chunk, tail)
CLAIMED_F64 = {(8192, 19, 4): (2, 1), (16384, 20, 2): (5, 5), (16384, 67, 2): (8, 3), (16384, 8, 2): (2, 2), (16384, 7, 2): (0, 0),
               (32768, 9, 2): (2, 1), (1 << 17, 5, 2): (1, 1), (1 << 18, 3, 2): (0, 0)}
EXTRA_16K = {64: (20, 8, 7), 32: (40, 16, 15)}  # every chunk under / the call on either side of the 8-row threshold


def batch_for(n, precision):
    if n in TABLE[precision]:
        return TABLE[precision][n]
    return -(-(1 << 20) // (n * precision // 8)) + 5  # 4 x batch x N x bytes >= 4 MiB, and 5 rows


def test_the_size_classes_cover_every_path_family(capi):
    reached = set()
    for precision in (64, 32):
        classes = size_classes(precision)
        reached |= set().union(*classes.values())
        assert len(classes) >= 6, classes
    assert reached >= REQUIRED, f"transform paths no size class reaches: {sorted(REQUIRED - reached)}"
    for key, want in CLAIMED_F64.items():
        n, batch, threads = key
        assert host_cut("transform", n, batch, 64, threads)[::2] == want, key
    # rows too long for a chunk are never cut
    for precision in (64, 32):
        n = 1 << MAX_LOG2[precision]
        assert all(host_cut("transform", n, b, precision, t) == (0, 0, 0) for b in range(1, 65) for t in (2, 4, 6, 16))


def _cases():
    out = []
    for precision in (64, 32):
        for L in range(1, MAX_LOG2[precision] + 1):
            out.append((precision, 1 << L, 0))
        out += [(precision, 16384, b) for b in EXTRA_16K[precision]]
    return out


@pytest.mark.parametrize("precision,n,batch", _cases(), ids=lambda v: str(v))
def test_transform_triangle(capi, oracle_mod, precision, n, batch):
    """batch = 0: the size's own batch (batch_for).  Every power of two up to the precision's limit runs, a superset of the
    library's size classes (which are known only with a device, after collection); a case is a few MiB."""
    if batch == 0:
        batch = batch_for(n, precision)
    capi.lib.pdsp_set_host_precision(precision)
    tol = 1e-12 if precision == 64 else 1e-5
    rng = np.random.default_rng(4242 + n + batch)
    re = rng.standard_normal((batch, n))
    im = rng.standard_normal((batch, n))
    plan = _plan(capi, n)
    try:
        cuts = regime(capi, "transform", plan, n, batch, precision)
        never = 2 * n * (precision // 8) > CHUNK_IN_BYTES
        small = 4 * batch * n * (precision // 8) < CHUNKED_MIN_BYTES
        rows = {0, batch - 1}
        for t in THREADS:
            per, workers, tail = cuts[t]
            if never or small:
                assert per == 0, (t, cuts[t])
                continue
            assert per >= 1 and workers >= 2 and 1 <= tail <= per, (t, cuts[t])
            if n in TABLE[precision] and TABLE[precision][n] == batch and per > 1:
                assert tail < per, f"the last chunk is not shorter: {cuts[t]} at {t} threads"
            # the first row of the last chunk, and a row on either side of the first chunk boundary
            rows |= {batch - tail, per - 1, per}
        rows = sorted(r for r in rows if 0 <= r < batch)
        rp, ip = _row_ptrs(re, C.c_double), _row_ptrs(im, C.c_double)
        oplan = oracle_mod.Plan(n)
        for kind, imag, inverse in (("real", None, 0), ("complex", im, 0), ("inverse", im, 1)):
            one = _transform(capi, plan, re, imag, inverse, 1)
            assert not np.isnan(one[0]).any() and not np.isnan(one[1]).any()
            for t in THREADS:
                got = _transform(capi, plan, re, imag, inverse, t)
                assert np.array_equal(one[0], got[0]) and np.array_equal(one[1], got[1]), \
                    f"{kind}: cut as {cuts[t]} on {t} threads differs from the one-shot sequence"
            ore, oim = np.full_like(re, np.nan), np.full_like(re, np.nan)
            capi.check(capi.lib.pdsp_fft_transform_rows_host_f64(plan, batch, n, rp, ip if imag is not None else None,
                                                                 capi.dptr(ore), capi.dptr(oim), inverse))
            assert np.array_equal(one[0], ore) and np.array_equal(one[1], oim), f"{kind}: the row-pointer form differs"
            for r in rows:
                row = _transform(capi, plan, re[r:r + 1], imag[r:r + 1] if imag is not None else None, inverse, 1)
                assert np.array_equal(one[0][r], row[0][0]) and np.array_equal(one[1][r], row[1][0]), \
                    f"{kind}: row {r} of {batch} differs from the one-row call (cuts {cuts})"
            chk = rows[:3]
            if inverse:
                wre, wim = oplan.inverse(re[chk], im[chk])
            elif imag is None:
                wre, wim = oplan.forward(re[chk])
            else:
                wre, wim = oplan.forward_complex(re[chk], im[chk])
            want = wre + 1j * wim
            have = one[0][chk] + 1j * one[1][chk]
            assert (np.abs(have - want).max(axis=1) / np.abs(want).max(axis=1)).max() <= tol
    finally:
        capi.lib.pdsp_plan_destroy(plan)


# ---- spectrum: the three batch forms against pdsp_spectrum_host_f64 ----------------------------------------------------

def _spectrum_one(capi, x, n, window, sides):
    bins = n // 2 + 1 if sides == 0 else n
    freq, amp, ph = np.full(bins, np.nan), np.full(bins, np.nan), np.full(bins, np.nan)
    peak = capi.Peak()
    capi.check(capi.lib.pdsp_spectrum_host_f64(capi.dptr(x), len(x), 48000.0, n, window, sides, capi.dptr(freq), capi.dptr(amp),
                                               capi.dptr(ph), C.byref(peak), None))
    return freq, amp, ph, np.array([peak.index, peak.frequency, peak.amplitude, peak.phase])


# N -> frames per precision: cut into chunks with a shorter last one (asserted below)
SPECTRUM_BATCH = {64: {16384: 19, 32768: 11, 1 << 17: 5}, 32: {16384: 37, 32768: 21, 1 << 17: 9}}


@pytest.mark.parametrize("precision,tol", [(64, 1e-12), (32, 1e-5)])
@pytest.mark.parametrize("sides", [0, 1])
@pytest.mark.parametrize("n", [16384, 32768, 1 << 17])
def test_spectrum_triangle(capi, oracle_mod, precision, tol, sides, n):
    capi.lib.pdsp_set_host_precision(precision)
    batch, window = SPECTRUM_BATCH[precision][n], 1  # hann
    rng = np.random.default_rng(77 + n + sides)
    t = np.arange(n)
    x32 = (rng.standard_normal((batch, n)) + 2.0 * np.sin(2 * np.pi * rng.integers(3, n // 4, (batch, 1)) * t / n)).astype(np.float32)
    x = x32.astype(np.float64)
    plan = _plan(capi, n)
    try:
        cuts = regime(capi, "spectrum", plan, n, batch, precision, sides)
    finally:
        capi.lib.pdsp_plan_destroy(plan)
    rows = {0, batch - 1}
    for th in THREADS:
        per, workers, tail = cuts[th]
        assert per >= 1 and workers >= 2 and 1 <= tail <= per and (tail < per or per == 1), (th, cuts[th])
        rows |= {batch - tail, per - 1, per}
    rows = sorted(r for r in rows if 0 <= r < batch)
    one = _spectrum_batch(capi, x, n, window, sides, 1)
    assert not any(np.isnan(a).any() for a in one)
    bins = n // 2 + 1 if sides == 0 else n
    for th in THREADS:
        got = _spectrum_batch(capi, x, n, window, sides, th)
        for a, b, what in zip(one, got, ("frequencies", "amplitude", "phase", "peaks")):
            assert np.array_equal(a, b), f"{what}: cut as {cuts[th]} on {th} threads differs from the one-shot sequence"
        for form, ptrs, fn in (("rows", _row_ptrs(x, C.c_double), capi.lib.pdsp_spectrum_rows_host_f64),
                               ("f32 rows", _row_ptrs(x32, C.c_float), capi.lib.pdsp_spectrum_rows_host_f32in)):
            freq, amp, ph = np.full(bins, np.nan), np.full((batch, bins), np.nan), np.full((batch, bins), np.nan)
            peaks = (capi.Peak * batch)()
            capi.check(fn(ptrs, batch, n, 48000.0, n, window, sides, capi.dptr(freq), capi.dptr(amp), capi.dptr(ph), peaks, None))
            pk = _peak_rows(capi, peaks)
            for a, b, what in zip(one, (freq, amp, ph, pk), ("frequencies", "amplitude", "phase", "peaks")):
                assert np.array_equal(a, b), f"{what}: the {form} form on {th} threads differs"
    kinds = ["rect", "hann", "hamming", "blackman"]
    for r in rows:
        f1, a1, p1, k1 = _spectrum_one(capi, x[r], n, window, sides)
        assert np.array_equal(one[0], f1) and np.array_equal(one[1][r], a1) and np.array_equal(one[2][r], p1) and \
            np.array_equal(one[3][r], k1), f"frame {r} of {batch} differs from pdsp_spectrum_host_f64 on it (cuts {cuts})"
    for r in rows[:3]:
        want = oracle_mod.spectrum(x[r], sample_rate=48000.0, fft_size=n, window=kinds[window], sides="one" if sides == 0 else "two")
        scale = np.abs(want["amplitude"]).max()
        assert np.abs(one[1][r] - want["amplitude"]).max() <= tol * scale
        assert np.array_equal(one[0], want["frequencies"])
        if sides == 0:
            assert int(one[3][r][0]) == want["peak"]["index"]

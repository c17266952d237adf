"""The sliding DFT on the MI355X held to its documented summation order, bit for bit and frame by frame
(pdsp_sdft_kernel.h, "THE SUMMATION ORDER"; sdft_ref.emulate(exact=True) restates it in numpy with a correctly rounded
fma, which test_sdft_exact_cpu.py holds to libm's).  test_gpu_sdft.py states the contract and the error bound; this
file imports its helpers unchanged and runs the kernel where that file does not reach:

  a  device = emulation on every frame at the sizes where the kernel changes shape (sdft_ref.PATH_SIZES: N < E, the
     one-wave boundary, f32's E = 4 / 8 switch, the first second round, N no multiple of E over several rounds, sixteen
     rounds of which the last holds one position, five components x sixteen rounds), six or three lengths each;
  b  hops that skip one, two and four chunks in a row, under the default tiles and tiles of 1, 2 and 3 chunks;
  c  hops from 2^31 - 1 to 2^63 - 1 (the host passes the kernel min(hop, T - N + 1)): one frame, three sentinels;
  d  the default tiles of 16 and of 8 chunks crossed; values of PDSP_SDFT_TILE_CHUNKS outside its range;
  e  256 bins, and the largest table the library accepts (2^21 entries), each checked bin against the bin alone;
  f  sentinels behind every series of the E = 8 and the multi-round stores;
  g  the case list of a reaches both f32 instantiations and the f64 one at 1, 2, 5 and 16 rounds.

Every comparison is on bit patterns (int32 / int64 views), over every frame.  Every test prints one SDFTBITS line --
the case, the count of differing values and the first differing (row, bin, frame) -- before it asserts.

The 64-bit branch of the kernel's frame-index division is taken when (s0 | hop) >> 32 != 0; with the hop the host
passes (<= T - N + 1) that needs a row of 2^32 samples, and no test here allocates one.
"""
import numpy as np
import pytest
import torch

import sdft_ref as R
from test_gpu_sdft import DEV, TORCH, cplx, tile_chunks

pytestmark = pytest.mark.gpu
DTYPES = ["f32", "f64"]
SENT = -12345.0


class Bits:
    """The differing values of one test; done() prints the SDFTBITS line, then asserts that there are none."""

    def __init__(self, case):
        self.case, self.count, self.total, self.first, self.checks = case, 0, 0, None, 0

    def add(self, got, want, where):
        """got, want: complex numpy [rows, K, F] of one precision."""
        assert got.shape == want.shape and got.dtype == want.dtype, (where, got.shape, want.shape)
        it = np.int32 if got.dtype == np.complex64 else np.int64
        g = np.stack([got.real, got.imag], axis=-1).view(it)
        w = np.stack([want.real, want.imag], axis=-1).view(it)
        bad = g != w
        self.checks += 1
        self.total += bad.size
        if bad.any() and self.first is None:
            self.first = (where,) + tuple(int(v) for v in np.argwhere(bad.any(axis=-1))[0])
        self.count += int(bad.sum())

    def ok(self, cond, where):
        self.checks += 1
        if not cond:
            self.count += 1
            self.first = self.first or (where, "condition")

    def done(self):
        print(f"SDFTBITS {self.case}: {self.count} of {self.total} values differ in {self.checks} checks; first at "
              f"(case, row, bin, frame) {self.first}")
        assert self.count == 0, self.first


def device(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(TORCH[dtype]).to(DEV)


def capi_planes(pdsp, s, xd, dtype, nbins, stride):
    """pdsp_sdft_<dtype> through the C ABI into sentinel-filled planes of out_stride `stride` with three values behind
    the last series: (re, im) as [rows, nbins, stride] and the two tails."""
    from pragma_dsp_amd import _capi, _device
    rows, t = xd.shape
    ore, oim = (torch.full((rows * nbins * stride + 3,), SENT, dtype=TORCH[dtype], device=DEV) for _ in range(2))
    _capi.check(getattr(_capi.lib, "pdsp_sdft_" + dtype)(s._h, rows, _device.ptr(xd), t, t, _device.ptr(ore),
                                                        _device.ptr(oim), stride, _device.stream_ptr(xd.device)))
    torch.cuda.synchronize()
    return [o[:-3].reshape(rows, nbins, stride) for o in (ore, oim)], [o[-3:] for o in (ore, oim)]


# ---- a: the device is the emulation ---------------------------------------------------------------------------------

A_CASES = [(n, w) for n in R.PATH_SIZES for w in R.path_windows(n)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,win", A_CASES)
def test_a_device_is_the_emulation_on_every_frame(pdsp, n, win, dtype):
    rows, bins = R.PATH_ROWS, R.path_bins(n)
    tally = Bits(f"a {dtype} N={n} {win} rows={rows} bins={len(bins)}")
    s = pdsp.SlidingDft(n, list(bins), hop=1, window=win)
    for t in R.path_lengths(n):
        got = cplx(*s.forward(device(R.signal(n, t)[:rows], dtype)))
        tally.add(got, R.emulated(n, t, win, dtype, rows, bins), f"T={t}")
    tally.done()


# ---- b: hops that skip chunks ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("win", ["rect", "hann"])
@pytest.mark.parametrize("n", [2049, 4096])
def test_b_hops_that_skip_chunks(pdsp, n, win, dtype):
    t, bins = 9 * n + 7, R.path_bins(n)
    xd = device(R.signal(n, t, seed=2)[:R.PATH_ROWS], dtype)
    base = cplx(*pdsp.SlidingDft(n, list(bins), hop=1, window=win).forward(xd))
    tally = Bits(f"b {dtype} N={n} {win}")
    for h in (2 * n, 2 * n + 5, 3 * n + 1, 5 * n):
        s = pdsp.SlidingDft(n, list(bins), hop=h, window=win)
        want = np.ascontiguousarray(base[..., ::h])
        assert s.frames(t) == want.shape[-1] >= 2
        for tc in (None, 1, 2, 3):
            with tile_chunks(tc):
                tally.add(cplx(*s.forward(xd)), want, f"hop={h} tiles={tc}")
    tally.done()


# ---- c: huge hops ---------------------------------------------------------------------------------------------------

HUGE = (2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 62, 2 ** 63 - 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [64, 2049])
def test_c_huge_hops_store_frame_zero_alone(pdsp, n, dtype):
    t, bins = 3 * n + 7, R.path_bins(n)
    xd = device(R.signal(n, t, seed=4)[:R.PATH_ROWS], dtype)
    tally = Bits(f"c {dtype} N={n}")
    for win in ("rect", "hann"):
        base = cplx(*pdsp.SlidingDft(n, list(bins), hop=1, window=win).forward(xd))[..., :1]
        for h in HUGE:
            s = pdsp.SlidingDft(n, list(bins), hop=h, window=win)
            assert s.hop == h and s.frames(t) == 1  # the handle keeps the caller's hop
            tally.add(cplx(*s.forward(xd)), base, f"{win} hop={h}")
            planes, tails = capi_planes(pdsp, s, xd, dtype, len(bins), 4)
            tally.add(cplx(planes[0][..., :1], planes[1][..., :1]), base, f"{win} hop={h} out_stride=4")
            tally.ok(all(bool((p[..., 1:] == SENT).all()) for p in planes) and
                     all(bool((q == SENT).all()) for q in tails), f"{win} hop={h} sentinels")
    tally.done()


# ---- d: the default tiles crossed -----------------------------------------------------------------------------------

def default_tile(n, dtype):
    """sdft_tile_chunks' default: 8 chunks where a chunk has more than one round, else 16."""
    return 8 if R.rounds_of(n, dtype) > 1 else 16


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("win", ["rect", "hann"])
@pytest.mark.parametrize("n,chunks,extra", [(64, 18, 5), (2049, 10, 3)])
def test_d_default_tiles_crossed(pdsp, n, chunks, extra, win, dtype):
    t, bins = chunks * n + extra, R.path_bins(n)
    # chunks with a start: more than one default tile, the last one partial
    assert default_tile(n, dtype) < (t - n) // n + 1 < 2 * default_tile(n, dtype)
    x = R.signal(n, t)[:R.PATH_ROWS]
    xd = device(x, dtype)
    s = pdsp.SlidingDft(n, list(bins), hop=1, window=win)
    tally = Bits(f"d {dtype} N={n} {win} T={t}")
    with tile_chunks(None):
        base = cplx(*s.forward(xd))
    tally.add(base, R.emulated(n, t, win, dtype, R.PATH_ROWS, bins), "default = emulation")
    for v in ("1", "0", "1048577", "x"):
        with tile_chunks(v):
            tally.add(cplx(*s.forward(xd)), base, f"PDSP_SDFT_TILE_CHUNKS={v}")
    tally.done()


# ---- e: many bins ---------------------------------------------------------------------------------------------------

def many_bins(n):
    """256 bins: fractional, negative and beyond N among them; bin 0 is 0 and bin 128 is 12.5."""
    b = (np.arange(256) - 128) * 0.40625 + 12.5
    b[0], b[255] = 0.0, n + 2.25
    return b


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,win,rows,extra,alone", [(64, "rect", 2, None, (0, 128, 255)), (64, "hann", 2, None, (0, 128, 255)),
                                                    (8191, "rect", 1, 300, (0, 255))])
def test_e_many_bins(pdsp, n, win, rows, extra, alone, dtype):
    t = 3 * n + 7 if extra is None else n + extra
    bins = many_bins(n)
    assert len(bins) * len(R.components(win)) * (n + 1) <= 1 << 21
    if n == 8191:
        assert len(bins) * (n + 1) == 1 << 21  # the largest handle the library accepts
    x = R.signal(n, t, seed=6)[:rows]
    xd = device(x, dtype)
    full = cplx(*pdsp.SlidingDft(n, bins, hop=1, window=win).forward(xd))
    assert full.shape == (rows, 256, R.frames_of(n, 1, t))
    tally = Bits(f"e {dtype} N={n} {win} K=256")
    for j in alone:
        one = cplx(*pdsp.SlidingDft(n, [bins[j]], hop=1, window=win).forward(xd))
        tally.add(one, full[:, j:j + 1], f"bin {j} alone")
    want = R.emulate(x, n, [bins[j] for j in alone], 1, win, dtype, exact=True)
    tally.add(np.ascontiguousarray(full[:, list(alone)]), want, "among 256 = emulation")
    tally.done()


def test_e_more_bins_than_the_limits_are_refused(pdsp):
    from pragma_dsp_amd import _capi
    for n, k, text in ((64, 257, "sliding DFT bins must be 1 ... 256, got 257"),
                       (8192, 256, "sliding DFT tables of 256 bins x 1 components x 8193 entries exceed 2^21 entries"),
                       (8191, 256, None)):
        if text is None:
            assert pdsp.SlidingDft(n, np.zeros(k)).bins.size == k
            continue
        with pytest.raises(pdsp.PdspError) as e:
            pdsp.SlidingDft(n, np.zeros(k))
        assert e.value.code == _capi.ERR_UNSUPPORTED_SIZE and str(e.value).startswith(text), str(e.value)
    print("SDFTBITS e refusals: 0 of 0 values differ in 3 checks; first at (case, row, bin, frame) None")


# ---- f: sentinels on the E = 8 and the multi-round stores -----------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("h", [1, 7])
@pytest.mark.parametrize("n", [2049, 16383])
def test_f_nothing_is_written_beyond_a_series(pdsp, n, h, dtype):
    t, bins = 3 * n + 7, [0.0, 12.5, n - 1.0]
    xd = device(R.signal(n, t)[:R.PATH_ROWS], dtype)
    s = pdsp.SlidingDft(n, bins, hop=h, window="hann")
    f = s.frames(t)
    assert f == R.frames_of(n, h, t)
    planes, tails = capi_planes(pdsp, s, xd, dtype, len(bins), f + 3)
    tally = Bits(f"f {dtype} N={n} hop={h} out_stride={f + 3}")
    tally.add(cplx(planes[0][..., :f], planes[1][..., :f]), cplx(*s.forward(xd)), "series")
    tally.ok(all(bool((p[..., f:] == SENT).all()) for p in planes), "the three values behind every series")
    tally.ok(all(bool((q == SENT).all()) for q in tails), "the three values behind the planes")
    tally.done()


# ---- g: what the table of a reaches ---------------------------------------------------------------------------------

def test_g_the_cases_of_a_reach_every_instantiation_and_round_count():
    """sdft_dev: f32 runs sdft_kernel<float, 4> up to N = 1024 and <float, 8> above, f64 <double, 4>; a chunk has
    ceil(N / 256 E) rounds.  From the case list alone."""
    reached = {(d, R.segment(n, d)) for n, _ in A_CASES for d in DTYPES}
    assert reached == {("f32", 4), ("f32", 8), ("f64", 4)}
    assert R.segment(1024, "f32") == 4 and R.segment(1025, "f32") == 8 and {1024, 1025} <= set(R.PATH_SIZES)
    rounds = {d: {R.rounds_of(n, d) for n, _ in A_CASES} for d in DTYPES}
    assert {1, 2, 5, 16} <= rounds["f64"] and {1, 2, 8} <= rounds["f32"]
    # the one live position of a last round, in either precision; five components at sixteen rounds
    assert R.rounds_of(2049, "f32") == 2 and 2049 - 256 * 8 == 1
    assert R.rounds_of(1025, "f64") == 2 and R.rounds_of(15361, "f64") == 16 and 15361 - 15 * 1024 == 1
    assert (16384, "blackman") in A_CASES and R.rounds_of(16384, "f64") == 16 and len(R.components("blackman")) == 5
    # N < E, and N no multiple of E over several rounds
    assert {2, 3} <= set(R.PATH_SIZES) and 5 in R.PATH_SIZES and all(n % 8 and R.rounds_of(n, "f32") > 1 for n in (4097, 16383))
    print(f"SDFTBITS g: 0 of 0 values differ; reached {sorted(reached)}, rounds f32 {sorted(rounds['f32'])} f64 "
          f"{sorted(rounds['f64'])}")

"""The state around the kernels (the boundary is synchronous and re-entrant): the host forms of every
family called from several threads at once, the plan cache of 16 entries under pressure and under
pdsp_plan_cache_clear(), the first call of a handle shared by four threads, and the life of every handle type --
create, call, destroy -- counted exactly by pdsp_dev_live_resources (include/pdsp_hip_dev.h).

Every comparison is bit equality or an exact counter: a result computed with other threads running must be the
single-threaded result bit for bit, and what a test created must be gone when it ends.  The single-threaded results
themselves are held once to the reference and the f64 bound of the family's own test module, imported from there.
Nothing depends on timing or on the device's free memory.  ctypes releases the GIL inside the C call, so the calls
really overlap."""
import gc
import threading

import numpy as np
import pytest
import torch

import ntt_ref
import pragma_dsp_amd as pd
import sdft_ref
import test_gpu_czt as czt_t
import test_gpu_dct as dct_t
import test_gpu_dft as dft_t
import test_gpu_dwt as dwt_t
import test_gpu_fir as fir_t
import test_gpu_hilbert as hil_t
import test_gpu_resample as res_t
import test_gpu_stft_pair as pair_t
import test_gpu_stft_paths as stft_t
from pragma_dsp_amd import _capi
from pragma_dsp_amd._capi import live_resources
from pragma_dsp_amd.batch import BatchedFft
from test_czt_cpu import GRID, grid_direct
from test_czt_cpu import row_err as czt_row_err
from test_dft_cpu import row_err as dft_row_err
from test_gpu_f64_dropin import f64_mode  # noqa: F401  (fixture: the host forms in their default f64 mode)
from test_hilbert_cpu import hilbert_ref
from test_resample_cpu import user_taps

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64 = torch.float64
HELD = ("cached_plans", "pinned", "tables", "table_bytes", "host_stage", "dev_stage", "streams")  # all but evictions


def flat(r):
    """A result of any host form as a tuple of arrays: what bit equality is asked of."""
    if isinstance(r, pd.SpectrumResult):
        return (r.frequencies, r.amplitude, r.phase,
                np.array([r.peak.index, r.peak.frequency, r.peak.amplitude, r.peak.phase], dtype=np.float64))
    if isinstance(r, (list, tuple)):
        return tuple(a for v in r for a in flat(v))
    if isinstance(r, torch.Tensor):
        return (r.contiguous().view(torch.int64).cpu().numpy() if r.dtype == torch.uint64 else r.cpu().numpy(),)
    return (np.asarray(r),)


def same_bits(a, b):
    a, b = flat(a), flat(b)
    return len(a) == len(b) and all(u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes()
                                    for u, v in zip(a, b))


def run_threads(target, count, timeout=120):
    """`count` daemon threads of target(tid, errors), joined with a timeout: none stuck, no error recorded."""
    assert count <= 8
    errors = []

    def body(tid):
        try:
            target(tid, errors)
        except Exception as exc:  # noqa: BLE001
            errors.append((tid, "exception", repr(exc)))

    threads = [threading.Thread(target=body, args=(t,), daemon=True) for t in range(count)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=timeout)
    assert not any(t.is_alive() for t in threads), "a worker is stuck"
    assert not errors, errors[:5]


def settled():
    """The counters with nothing of this process pending: unreachable handles of earlier tests collected, the plan
    cache empty (no call is in flight, so nothing is pinned and the clear frees every entry)."""
    gc.collect()
    assert pd.lib.pdsp_plan_cache_clear() == 0
    torch.cuda.synchronize()
    live = live_resources()
    assert live["cached_plans"] == 0 and live["pinned"] == 0
    return live


def held(live):
    return {k: live[k] for k in HELD}


# ---- a. the host forms in parallel -----------------------------------------------------------------------------------

def host_cases():
    """name -> (call, check): the call of one host form on fixed data, and the check that holds its single-threaded
    result to the family's own reference and f64 bound."""
    rng = np.random.default_rng(2024)
    cases = {}
    lg = 7  # log2 128

    x = rng.standard_normal((3, 128))

    def dct_check(inverse):
        def check(got):
            want = (dct_t.idct_ref if inverse else dct_t.dct_ref)(x, 2, "ortho")
            assert dct_t.rel_rows(got, want) <= dct_t.TOL["f64"] * lg
        return check
    cases["dct"] = (lambda: pd.dct(x, type=2, norm="ortho"), dct_check(False))
    cases["idct"] = (lambda: pd.idct(x, type=2, norm="ortho"), dct_check(True))

    xh = rng.standard_normal((3, 100))  # len 100: the plan of 128 points
    a_ref = hilbert_ref(xh, 128)
    for name, fn, mode in (("hilbert", pd.hilbert, "analytic"), ("envelope", pd.envelope, "envelope"),
                           ("instantaneous_phase", pd.instantaneous_phase, "phase")):
        def hil_check(got, mode=mode):
            assert got.shape == (3, 128)
            assert hil_t.err_rows(got, a_ref, mode) <= hil_t.bound("f64", 128, mode)
        cases[name] = (lambda fn=fn: fn(xh, 128), hil_check)

    xf, taps = rng.standard_normal(500), rng.standard_normal(9)

    def fir_check(got):
        assert got.shape == (508,)
        assert fir_t.err(got, fir_t.ref_full(xf, taps), xf, taps) <= fir_t.TOL[F64]
    cases["firFilter"] = (lambda: pd.firFilter(xf, taps, "full"), fir_check)

    xs = rng.standard_normal(400)  # fftSize 128, hop 32: 9 frames
    frames = 1 + (400 - 128) // 32
    spec = rng.standard_normal((frames, 65)) + 1j * rng.standard_normal((frames, 65))
    plan128 = BatchedFft(128, DEV, F64)
    w = pair_t.win64(plan128, "hann")
    plan128.close()

    def stft_check(got):
        want = pair_t.ref_stft(xs, 128, 32, w)
        assert got.shape == want.shape
        assert np.abs(got - want).max() / np.abs(want).max() <= pair_t.FWD_TOL[F64] * lg

    def istft_check(got):
        want, den, ymax = pair_t.ref_istft(spec, 128, 32, w)
        assert got.shape == want.shape and stft_t.zeros_where_den_small(got, den)
        assert stft_t.inv_err(got, want, den, ymax, 128, 32) <= pair_t.INV_TOL[F64] * lg
    cases["stft"] = (lambda: pd.stft(xs, 128, 32, "hann"), stft_check)
    cases["istft"] = (lambda: pd.istft(spec, 32, "hann"), istft_check)

    for ln in (17, 100):  # 2M = 128 and 512
        z = rng.standard_normal((3, ln)) + 1j * rng.standard_normal((3, ln))

        def dft_check(got, z=z, ln=ln, ref=np.fft.fft):
            assert dft_row_err(got, ref(z)) <= dft_t.bound("f64", ln)
        cases[f"dft{ln}"] = (lambda z=z: pd.dft(z), dft_check)
        cases[f"idft{ln}"] = (lambda z=z: pd.idft(z), lambda got, z=z, ln=ln: dft_check(got, z, ln, np.fft.ifft))

    zc = rng.standard_normal((3, 33)) + 1j * rng.standard_normal((3, 33))  # L = 33, K = 32: M = 64

    def czt_check(got):
        assert czt_row_err(got, grid_direct(zc, 32, GRID // 32), zc) <= czt_t.bound("f64", 33, 32)

    def zoom_check(got):  # the band [0.25, 0.75) of fs = 2 in 32 points: step = 1 / 128, start = 1 / 8
        assert czt_row_err(got, grid_direct(zc, 32, GRID // 128, GRID // 8), zc) <= czt_t.bound("f64", 33, 32)
    cases["czt"] = (lambda: pd.czt(zc, 32), czt_check)
    cases["zoom_fft"] = (lambda: pd.zoom_fft(zc, [0.25, 0.75], 32), zoom_check)

    cs = dwt_t.case(96, 3, "db2", F64, 3)
    cases["wavedecHost"] = (lambda: pd.wavedecHost(cs["x"], "db2", 3),
                            lambda got: dwt_t.hold(got, cs["fwd"], cs["fwd_bound"], "wavedecHost"))
    cases["waverecHost"] = (lambda: pd.waverecHost(cs["c"], "db2", 3),
                            lambda got: dwt_t.hold(got, cs["inv"], cs["inv_bound"], "waverecHost"))

    rows = ntt_ref.rows(64, 3)
    xn = np.array(rows, dtype=np.uint64)
    fwd = ntt_ref.transform_rows(rows)
    xk = np.array(fwd, dtype=np.uint64)

    def ntt_check(got):
        assert got.dtype == np.uint64 and got.tolist() == fwd

    def intt_check(got):
        assert got.tolist() == [[v % ntt_ref.P for v in r] for r in rows]
    cases["ntt"] = (lambda: pd.ntt(xn), ntt_check)
    cases["intt"] = (lambda: pd.intt(xk), intt_check)
    pa, pb = xn[:, :30], xn[0, :20]  # 30 + 20 - 1 = 49 coefficients on the transform of 64 points

    def polymul_check(got):
        assert got.tolist() == [ntt_ref.cyclic(rows[r][:30], rows[0][:20], 64)[:49] for r in range(3)]
    cases["polymul"] = (lambda: pd.polymul(pa, pb), polymul_check)
    ia, ib = rng.integers(-10 ** 6, 10 ** 6, (2, 40)), rng.integers(-10 ** 6, 10 ** 6, 25)  # 64 outputs: n = 64

    def exact_check(got):
        assert got.dtype == np.int64 and all(np.array_equal(got[r], np.convolve(ia[r], ib)) for r in range(2))
    cases["convolve_exact"] = (lambda: pd.convolve_exact(ia, ib), exact_check)

    xd = sdft_ref.signal(24, 200, seed=5)  # window 24, 200 samples
    bins = [0.0, 3.5, -2.0]

    def sdft_check(got):
        re, im = sdft_ref.direct(xd, 24, bins, 3, "hann")
        assert sdft_ref.err_units(got, re, im, 24, "f64", np.abs(xd).max()) <= sdft_ref.BOUND["f64"]

    def goertzel_check(got):
        re, im = sdft_ref.direct(xd[:, :24], 24, bins)
        assert sdft_ref.err_units(got[..., None], re, im, 24, "f64", np.abs(xd).max()) <= sdft_ref.BOUND["f64"]
    cases["sliding_dft"] = (lambda: pd.sliding_dft(xd, 24, bins, hop=3, window="hann"), sdft_check)
    cases["goertzel"] = (lambda: pd.goertzel(xd[:, :24], bins), goertzel_check)

    xr, h17 = res_t.signal((3, 100), F64, 77), user_taps(17)  # 3/2, 100 samples

    def resample_check(make, what):
        def check(got):  # the device form is held to the module's reference and bound; the host form is its bits
            r = make()
            y = res_t.check(r, xr, F64, what)
            r.close()
            assert np.array_equal(got, y.cpu().numpy())
        return check
    cases["resamplePoly"] = (lambda: pd.resamplePoly(xr, 3, 2),
                             resample_check(lambda: pd.Resampler(3, 2, device=DEV, dtype=F64), "resamplePoly"))
    cases["upfirdnHost"] = (lambda: pd.upfirdnHost(h17, xr, 3, 2),
                            resample_check(lambda: pd.Upfirdn(h17, 3, 2, device=DEV, dtype=F64), "upfirdnHost"))

    xp = rng.standard_normal((4, 128))
    opts = {"sampleRate": 48000, "fftSize": 128, "window": "hann"}

    def spectrum_check(oracle_mod):
        def check(got):  # tests/test_gpu_f64_dropin.py, test_spectrum_matches_oracle_to_f64_rounding
            for g, row in zip(got if isinstance(got, list) else [got], xp):
                want = oracle_mod.spectrum(row, sample_rate=48000, window="hann")
                assert np.abs(g.amplitude - want["amplitude"]).max() <= 1e-13 * max(1.0, want["amplitude"].max())
                assert np.array_equal(g.frequencies, want["frequencies"])
        return check
    cases["spectrum"] = (lambda: pd.spectrum(xp[0], opts), spectrum_check)
    cases["spectrumBatch"] = (lambda: pd.spectrumBatch(list(xp), opts), spectrum_check)
    return cases


def test_a_host_forms_in_parallel_give_the_single_threaded_bits(f64_mode, oracle_mod):  # noqa: F811
    start = settled()
    cases = host_cases()
    want = {}
    for name, (call, check) in cases.items():  # single-threaded first, each held once to its reference
        want[name] = call()
        (check(oracle_mod) if name.startswith("spectrum") else check)(want[name])
        assert same_bits(call(), want[name]), name  # and repeatable before any thread starts
    names = list(cases)
    assert len(names) == 26
    threads, rounds = 6, 20

    def worker(tid, errors):
        off = tid * len(names) // threads
        for rnd in range(rounds):
            for i in range(len(names)):
                name = names[(off + i) % len(names)]
                if not same_bits(cases[name][0](), want[name]):
                    errors.append((tid, rnd, name))
                    return

    run_threads(worker, threads)
    mid = live_resources()
    print(f"REENTRANT a: {len(names)} host forms x {threads} threads x {rounds} rounds; afterwards {mid}")
    assert mid["pinned"] == 0 and mid["cached_plans"] <= 16
    end = settled()
    assert held(end) == held(start)  # the per-call handles of dft, czt, dwt, ntt, sdft and the resamplers are gone


# ---- b. the cache under pressure -------------------------------------------------------------------------------------

SIZES = [1 << k for k in range(17)]  # 17 sizes on one device: one more than the cache holds


def test_b_the_plan_cache_under_pressure_and_under_clear(f64_mode):  # noqa: F811
    start = settled()
    rng = np.random.default_rng(17)
    x = {n: rng.standard_normal(n) for n in SIZES}

    def call(n):
        return pd.spectrum(x[n], {"sampleRate": 48000, "fftSize": n, "window": "hann"})

    first, tables = {}, []
    for rnd in range(3):  # round robin: from the 17th call on every call misses and evicts the size that comes next
        for n in SIZES:
            got = call(n)
            if rnd == 0:
                first[n] = got
            assert same_bits(got, first[n]), (rnd, n)
            live = live_resources()
            assert live["cached_plans"] <= 16 and live["pinned"] == 0, (rnd, n, live)
        tables.append(live_resources())
    for rnd, live in enumerate(tables):
        print(f"REENTRANT b: after pass {rnd + 1} of {len(SIZES)} sizes {live}")
    assert tables[0]["cached_plans"] == 16
    # least recently used first, so one eviction in the first pass and 17 in each later one
    assert tables[2]["evictions"] - start["evictions"] == 1 + 17 + 17
    assert held(tables[2]) == held(tables[1])  # the same 16 plans, windows, staging buffers and streams: nothing piles up

    threads, rounds = 6, 3
    stop = threading.Event()
    clears = []

    def worker(tid, errors):
        if tid == threads:  # the seventh thread clears the cache until the others are done
            while not stop.is_set():
                clears.append(pd.lib.pdsp_plan_cache_clear())
            return
        try:
            order = SIZES[3 * tid:] + SIZES[:3 * tid]
            if tid % 2:
                order = order[::-1]
            for rnd in range(rounds):
                for n in order:
                    if not same_bits(call(n), first[n]):
                        errors.append((tid, rnd, n))
                        return
        finally:
            done.append(tid)
            if len(done) == threads:
                stop.set()

    done = []
    try:
        run_threads(worker, threads + 1)
    finally:
        stop.set()
    after = live_resources()
    print(f"REENTRANT b: {threads} threads x {rounds} rounds x {len(SIZES)} sizes against {len(clears)} clears; afterwards {after}")
    assert clears and not any(clears), f"{sum(1 for c in clears if c)} of {len(clears)} clears failed"
    assert after["pinned"] == 0
    end = settled()  # the final clear: no cached plan is left
    assert held(end) == held(start)


# ---- c. the first use of a shared handle -----------------------------------------------------------------------------

def f32(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def first_use_cases():
    """name -> (make, inputs of four threads (numpy), call(handle, device tensors)): tables uploaded on first use
    (Resampler, Upfirdn, Dwt, Ntt, a plan's windows) and at create (SlidingDft, Dft, Czt)."""
    rng = np.random.default_rng(31)
    h17 = user_taps(17)
    words = [np.array(ntt_ref.rows(64, 2, start=t), dtype=np.uint64).view(np.int64) for t in range(4)]

    def windowed(p, x):
        return p.spectrum(x, p.window("hann"), want_phase=True)[:2]
    return {
        "Resampler": (lambda: pd.Resampler(3, 2, device=DEV), [f32(rng, 2, 100) for _ in range(4)], lambda r, x: r.apply(x)),
        "Upfirdn": (lambda: pd.Upfirdn(h17, 3, 2, device=DEV), [f32(rng, 2, 100) for _ in range(4)], lambda r, x: r.apply(x)),
        "Dwt-f32": (lambda: pd.Dwt("db2", 3, DEV), [f32(rng, 2, 96) for _ in range(4)], lambda w, x: w.forward(x)),
        "Dwt-f64": (lambda: pd.Dwt("db2", 3, DEV, F64), [rng.standard_normal((2, 96)) for _ in range(4)],
                    lambda w, x: w.forward(x)),
        "Ntt": (lambda: pd.Ntt(64, DEV), words, lambda h, x: h.forward(x.view(torch.uint64))),
        "SlidingDft": (lambda: pd.SlidingDft(24, [0.0, 3.5, -2.0], 3, "hann", DEV), [f32(rng, 2, 200) for _ in range(4)],
                       lambda s, x: s.forward(x)),
        "BatchedFft.window": (lambda: BatchedFft(128, DEV), [f32(rng, 5, 128) for _ in range(4)], windowed),
        "Dft": (lambda: pd.Dft(100, DEV), [f32(rng, 2, 2, 100) for _ in range(4)], lambda d, x: d.forward(x[0], x[1])),
        "Czt": (lambda: pd.Czt(33, 32, 1.0 / 32, device=DEV), [f32(rng, 2, 33) for _ in range(4)],
                lambda c, x: c.forward(x)),
    }


@pytest.mark.parametrize("name", ["Resampler", "Upfirdn", "Dwt-f32", "Dwt-f64", "Ntt", "SlidingDft", "BatchedFft.window",
                                  "Dft", "Czt"])
def test_c_first_use_of_a_shared_handle(name):
    start = settled()
    make, inputs, call = first_use_cases()[name]
    ref = make()  # a second handle, used single-threaded beforehand
    want = [flat(call(ref, torch.from_numpy(a).to(DEV))) for a in inputs]
    ref.close()
    handles = [make() for _ in range(16)]
    barrier = threading.Barrier(4)

    def worker(tid, errors):
        try:
            stream = torch.cuda.Stream(DEV)
            with torch.cuda.stream(stream):
                x = torch.from_numpy(inputs[tid]).to(DEV)  # its own buffers, ordered on its own stream
                for i, h in enumerate(handles):
                    barrier.wait(timeout=60)  # the four first calls of handle i leave together
                    out = call(h, x)
                    stream.synchronize()
                    if not same_bits(out, want[tid]):
                        errors.append((name, tid, i))
        except threading.BrokenBarrierError:
            errors.append((name, tid, "the barrier broke: another worker failed or is stuck"))
        except Exception:
            barrier.abort()
            raise

    run_threads(worker, 4)
    peak = live_resources()
    print(f"REENTRANT c: {name}: 16 handles after their first calls hold {peak['tables'] - start['tables']} tables, "
          f"{peak['table_bytes'] - start['table_bytes']} bytes")
    for h in handles:
        h.close()
    end = settled()
    assert (end["tables"], end["table_bytes"]) == (start["tables"], start["table_bytes"])
    assert held(end) == held(start)


# ---- d. churn of every handle type -----------------------------------------------------------------------------------

def churn_cases():
    """name -> one cycle: create, one call, destroy -- or one call of a host form that does all three itself."""
    rng = np.random.default_rng(43)
    dev = lambda *shape: torch.from_numpy(f32(rng, *shape)).to(DEV)  # noqa: E731
    x100, x33, x96, x200, x128, x500 = dev(2, 100), dev(2, 33), dev(2, 96), dev(2, 200), dev(2, 128), dev(2, 500)
    words = torch.from_numpy(np.array(ntt_ref.rows(64, 2), dtype=np.uint64).view(np.int64)).to(DEV).view(torch.uint64)
    taps = rng.standard_normal(9)
    z100, z33 = rng.standard_normal((2, 100)) + 0j, rng.standard_normal((2, 33)) + 0j
    h100, h96 = rng.standard_normal((2, 100)), rng.standard_normal((2, 96))

    def handle(make, call):
        def cycle():
            h = make()
            call(h)
            h.close()
        return cycle

    def fir():
        f = pd.FirFilter(taps, DEV)
        f.apply(x500)
        f.plan.close()

    def plan():
        p = BatchedFft(128, DEV)
        p.dct(x128)
        p.hilbert(x128[:, :100])
        p.close()
    return {
        "Dft": handle(lambda: pd.Dft(100, DEV), lambda d: d.forward(x100)),
        "Czt": handle(lambda: pd.Czt(33, 32, 1.0 / 32, device=DEV), lambda c: c.forward(x33)),
        "Dwt": handle(lambda: pd.Dwt("db2", 3, DEV), lambda w: w.forward(x96)),
        "Ntt": handle(lambda: pd.Ntt(64, DEV), lambda h: h.forward(words)),
        "SlidingDft": handle(lambda: pd.SlidingDft(24, [0.0, 3.5], 3, "hann", DEV), lambda s: s.forward(x200)),
        "Resampler": handle(lambda: pd.Resampler(3, 2, device=DEV), lambda r: r.apply(x100)),
        "FirFilter": fir,
        "BatchedFft": plan,
        "dft": lambda: pd.dft(z100),
        "czt": lambda: pd.czt(z33, 32),
        "resamplePoly": lambda: pd.resamplePoly(h100, 3, 2),
        "wavedecHost": lambda: pd.wavedecHost(h96, "db2", 3),
    }


@pytest.mark.parametrize("name", ["Dft", "Czt", "Dwt", "Ntt", "SlidingDft", "Resampler", "FirFilter", "BatchedFft", "dft",
                                  "czt", "resamplePoly", "wavedecHost"])
def test_d_churn_hands_everything_back(name, f64_mode):  # noqa: F811
    cycle = churn_cases()[name]
    cycle()  # the host forms' cached plans of this case exist before the first reading
    gc.collect()
    torch.cuda.synchronize()
    before = live_resources()
    seen = set()
    for i in range(300):
        cycle()
        if i % 50 == 0:
            seen.add(live_resources()["tables"])
    gc.collect()
    torch.cuda.synchronize()
    after = live_resources()
    print(f"REENTRANT d: {name}: 300 cycles, before and after {after}")
    assert after == before, name  # every counter, the evictions too: 300 cycles reuse the plans the first one cached
    assert seen == {before["tables"]}, (name, seen)  # and level in between, not only at the end


# ---- e. closed handles -----------------------------------------------------------------------------------------------

def closed_cases():
    """name -> (make, calls after close()): every handle class of the package and every method that reaches the library
    with the handle."""
    rng = np.random.default_rng(59)
    dev = lambda *shape: torch.from_numpy(f32(rng, *shape)).to(DEV)  # noqa: E731
    x100, x33, x96, x200, x128 = dev(2, 100), dev(2, 33), dev(2, 96), dev(2, 200), dev(2, 128)
    z128 = torch.complex(x128, x128)
    sig, bins128 = dev(400), dev(9, 65)
    words = torch.from_numpy(np.array(ntt_ref.rows(64, 2), dtype=np.uint64).view(np.int64)).to(DEV).view(torch.uint64)
    w30, w20 = words.view(torch.int64)[:, :30].view(torch.uint64), words.view(torch.int64)[0, :20].view(torch.uint64)
    h17 = user_taps(17)
    return {
        "BatchedFft": (lambda: BatchedFft(128, DEV), [
            lambda p: p.forward(x128), lambda p: p.forward(x128, x128), lambda p: p.inverse(x128, x128),
            lambda p: p.forward_interleaved(z128), lambda p: p.inverse_interleaved(z128), lambda p: p.window("hann"),
            lambda p: p.spectrum(x128), lambda p: p.spectrum(x128, "hann"), lambda p: p.spectrum_peaks(x128),
            lambda p: p.stft(sig, 32, "rect"), lambda p: p.stft_complex(sig, 32, "rect"),
            lambda p: p.stft_complex(sig, 32, "hann"), lambda p: p.istft(bins128, bins128, 32, "rect"),
            lambda p: p.dct(x128), lambda p: p.idct(x128), lambda p: p.hilbert(x128), lambda p: p.hilbert_imag(x128),
            lambda p: p.envelope(x128), lambda p: p.instantaneous_phase(x128)]),
        "Resampler": (lambda: pd.Resampler(3, 2, device=DEV), [lambda r: r.apply(x100), lambda r: r.output_len(100)]),
        "Upfirdn": (lambda: pd.Upfirdn(h17, 3, 2, device=DEV), [lambda r: r.apply(x100), lambda r: r.output_len(100)]),
        "Dft": (lambda: pd.Dft(100, DEV), [lambda d: d.forward(x100), lambda d: d.inverse(x100, x100)]),
        "Czt": (lambda: pd.Czt(33, 32, 1.0 / 32, device=DEV), [lambda c: c.forward(x33)]),
        "Dwt": (lambda: pd.Dwt("db2", 3, DEV), [lambda w: w.forward(x96), lambda w: w.inverse(x96)]),
        "Ntt": (lambda: pd.Ntt(64, DEV), [lambda h: h.forward(words), lambda h: h.inverse(words),
                                          lambda h: h.convolve(w30, w20)]),
        "SlidingDft": (lambda: pd.SlidingDft(24, [0.0, 3.5], 3, "hann", DEV), [lambda s: s.forward(x200)]),
    }


@pytest.mark.parametrize("name", ["BatchedFft", "Resampler", "Upfirdn", "Dft", "Czt", "Dwt", "Ntt", "SlidingDft"])
def test_e_a_closed_handle_refuses_every_call(name):
    """Every entry point that takes a handle checks it for null before anything else (the pdsp_capi*.hip units: check_plan_batch,
    check_packed_plan, upfirdn_t, dft_t, czt_t, dwt_t, ntt_t, sdft_t, pdsp_plan_window_*), and close() leaves the
    Python object with a null handle: a call after close() is an argument error, not a crash."""
    make, calls = closed_cases()[name]
    gc.collect()
    before = live_resources()
    h = make()
    for call in calls:  # each works on the open handle
        call(h)
    torch.cuda.synchronize()
    h.close()
    assert live_resources() == before
    h.close()  # twice: a no-op
    assert live_resources() == before
    for i, call in enumerate(calls):
        with pytest.raises(pd.PdspError) as e:
            call(h)
        assert e.value.code == _capi.ERR_BAD_ARG, (name, i, str(e.value))
        assert "null" in str(e.value), (name, i, str(e.value))
    assert live_resources() == before
    h.close()
    assert h._h is None
    # a FirFilter whose plan is closed refuses too (its plan is the handle it calls with)
    if name == "BatchedFft":
        f = pd.FirFilter(np.ones(9), DEV)
        x = torch.zeros(2, 500, device=DEV)
        f.apply(x)
        f.plan.close()
        with pytest.raises(pd.PdspError) as e:
            f.apply(x)
        assert e.value.code == _capi.ERR_BAD_ARG and "null" in str(e.value)
        assert live_resources() == before

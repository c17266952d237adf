"""Graph capture and replay of every stream-taking entry point ("Streams and graphs").

The contract: a call that draws no stream-ordered scratch, on a handle that has made one eager call in the precision
(and, for a named window, after plan.window(kind)), makes only kernel launches on the stream it is given.  During a
capture nothing executes, so whatever an entry point enqueued on another stream would either run at once -- an output
changes while the graph is being recorded -- or be missing from the graph -- a replay on fresh inputs returns stale
outputs.  A sentinel shows either.  Every row of tests/graph_capture_cases.py goes through the same six steps:

  1. two eager calls, on inputs A and then B, their outputs kept; during the first the modules' `lib` is a recording
     proxy, and the stream entry points reached must be exactly the ones the row declares;
  2. the eager result on A against the family's own f64 reference at the family's own bound, both imported from the
     family's test module: replay equality below is bitwise, this only shows the eager result at this shape is right;
  3. the outputs filled with a sentinel (NaN; a fixed odd pattern for integers), then the call captured on a side
     stream -- one stream, no events, forks or joins -- after which every output still holds the sentinel;
  4. a replay, whose output bits must equal the eager bits on A;
  5. B copied over the input buffers in place, the outputs refilled, a replay: the eager bits on B.  This is the step
     that catches work left out of the graph and values baked in from the host at capture time;
  6. two more replays with the same bits, and pdsp_dev_live_resources unchanged since step 3: capture and replay
     upload, allocate and create nothing.
Where an API has no `out=`, the tensors returned inside the capture are kept, filled with the sentinel before each
replay and compared in steps 4 to 6.

The refusal (contract point 2): a call that would have to upload its table on a capturing stream raises PdspError
"stream is capturing: ..." before any HIP call a capture forbids, and the caller's capture stays valid."""
import ctypes as C
import gc
import importlib
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import graph_capture_cases as G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODULES = ("batch", "filters", "dft", "czt", "resample", "wavelet", "ntt", "sdft")  # each has its own `lib`
SENT_I32 = 0x5A5A5A5B
SENT_I64 = 0x5A5A5A5A5A5A5A5B
SINGLE_PASS_TRANSFORM = {1, 2, 3, 4, 5, 6}   # include/pdsp_hip_dev.h, PDSP_DEV_PATH_INFO [0]: one rows kernel
SINGLE_PASS_SPECTRUM = {13, 14, 15, 16, 17}  # one spectrum kernel, no scratch plane pairs
PATH, PAIRS, WMODE, FUSED_PEAKS = 0, 9, 12, 14
STREAM_ENTRIES = frozenset(G.stream_entry_points())


def _t(dt):
    return torch.float32 if dt == "f32" else torch.float64


def _np(dt):
    return np.float32 if dt == "f32" else np.float64


def rounded(a, dt):
    """f64 values that the dtype holds exactly."""
    return np.asarray(a, np.float64).astype(_np(dt)).astype(np.float64)


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_t(dt)).to(DEV)


def raw(t):
    """The tensor's bits as integers of the same width (a complex tensor: of its parts); views keep their strides."""
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64)


def is_int(t):
    return not (t.is_floating_point() or t.is_complex())


def fill_sentinel(ts):
    for t in ts:
        if is_int(t):
            raw(t).fill_(SENT_I32 if t.element_size() == 4 else SENT_I64)
        else:
            (torch.view_as_real(t) if t.is_complex() else t).fill_(float("nan"))


def holds_sentinel(t):
    if is_int(t):
        return bool((raw(t) == (SENT_I32 if t.element_size() == 4 else SENT_I64)).all())
    return bool(torch.isnan(torch.view_as_real(t) if t.is_complex() else t).all())


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(raw(a), raw(b))


def load(bufs, arrays):
    """Host arrays over the input buffers, in place."""
    for buf, a in zip(bufs, arrays):
        a = np.array(a)  # a writable copy: some families share read-only cases
        if a.dtype == np.uint64:
            raw(buf).copy_(torch.from_numpy(a.view(np.int64)))
        else:
            buf.copy_(torch.from_numpy(a).to(buf.dtype))


class RecordingLib:
    """Forwards to the real library and keeps the names of the functions called."""

    def __init__(self, real):
        self._real, self.names = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("pdsp_"):
            return fn

        def call(*args):
            self.names.append(name)
            return fn(*args)
        return call


def clones(ts):
    return [raw(t).clone().view(t.dtype) if t.dtype == torch.uint64 else t.clone() for t in ts]


def path_info(dt, spectrum, *args):
    """PDSP_DEV_PATH_INFO of the path query for a call with these arguments."""
    from pragma_dsp_amd import _capi
    info = (C.c_int * 17)(*([-1] * 17))
    fn = getattr(_capi.lib, f"pdsp_dev_{'spectrum' if spectrum else 'transform'}_path_{dt}")
    _capi.check(fn(*args, info))
    return list(info)


_SIDE = []


def side_stream():
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream(DEV))
    return _SIDE[0]


class _Worst:
    """What the path files' check functions record into; nothing is reported from here."""

    def __init__(self):
        self.w = {}

    def add(self, kind, n, errs):
        return float(np.max(errs))


# ---- the builders: handle, inputs A and B, outputs, the call, the reference check, the single-pass guard -------------
# A builder returns: ins (input buffers), make(seed) (host arrays for them), outs (the preallocated outputs, each
# passed through `out=`), call() (-> every output tensor of the call), check(eager outputs on A), guard(outputs).

def _paths(dt):
    return importlib.import_module("test_gpu_f32_paths" if dt == "f32" else "test_gpu_f64_paths")


def build_fft(r):
    from pragma_dsp_amd.batch import BatchedFft
    import test_gpu_f32_paths as F32
    n, rows = r.shape
    p = BatchedFft(n, DEV, _t(r.dt))
    cplx = r.op != "real"
    inter = r.op in ("ifwd", "iinv")
    kind = "inv" if r.op in ("inverse", "iinv") else "fwd"
    state = {}

    def make(seed):
        re, im = F32.make_rows(np.random.default_rng([n, rows, seed]), rows, n, cplx, first=seed)
        if seed == 0:
            state["re"], state["im"] = re, im
        return [re + 1j * im] if inter else ([re, im] if cplx else [re])

    if inter:
        ins = [torch.empty((rows, n), dtype=torch.complex64 if r.dt == "f32" else torch.complex128, device=DEV)]
        outs = [torch.empty_like(ins[0])]
        call = lambda: [p.forward_interleaved(ins[0], out=outs[0], inverse=r.op == "iinv")]  # noqa: E731
    else:
        ins = [torch.empty((rows, n), dtype=_t(r.dt), device=DEV) for _ in range(2 if cplx else 1)]
        outs = [torch.empty((rows, n), dtype=_t(r.dt), device=DEV) for _ in range(2)]
        if r.op == "inverse":
            call = lambda: list(p.inverse(ins[0], ins[1], out=tuple(outs)))  # noqa: E731
        else:
            call = lambda: list(p.forward(ins[0], ins[1] if cplx else None, out=tuple(outs)))  # noqa: E731

    def check(eager):
        P = _paths(r.dt)
        if r.dt == "f64":
            P.check_long_double()
        if inter:
            got = eager[0].cpu().numpy().astype(np.complex128)
        else:
            got = eager[0].double().cpu().numpy() + 1j * eager[1].double().cpu().numpy()
        ref = P.reference_transform(r.op, state["re"], state["im"])
        errs = P.row_errors(got, ref)
        print(f"CAPTURE {r.name}: eager error {errs.max():.3e}, bound {P.bound(kind, n):.3e}")
        assert errs.max() <= P.bound(kind, n), (r.name, errs)
        zero = np.all(ref == 0, axis=-1)
        assert (got[zero] == 0).all()

    def guard(outputs):
        if inter:  # no path query takes interleaved rows: the entry points refuse every size that is not single-pass
            assert n <= (16384 if r.dt == "f32" else 8192)
            return
        info = path_info(r.dt, False, p._h, rows, ins[0].data_ptr(), ins[1].data_ptr() if cplx else None,
                         outs[0].data_ptr(), outs[1].data_ptr(), int(r.op == "inverse"))
        assert info[PATH] in SINGLE_PASS_TRANSFORM and info[PAIRS] == 0, info

    return SimpleNamespace(ins=ins, make=make, outs=outs, call=call, check=check, guard=guard, keep=p)


def _spectrum_outputs(eager_amp, eager_ph, eager_pk):
    out = {}
    if eager_amp is not None:
        out["amp"] = eager_amp.cpu().numpy()
    if eager_ph is not None:
        out["ph"] = eager_ph.cpu().numpy()
    if eager_pk is not None:
        out["idx"] = eager_pk.cpu().numpy().reshape(-1, 1)
    return out


def _check_spectrum(r, n, frames, out, window, sides):
    P = _paths(r.dt)
    if r.dt == "f64":
        P.check_long_double()
    fails = P.check_spectrum(_Worst(), n, frames, out, window, sides, r.name)
    assert not fails, fails


def _table_window(dt, n, kind):
    """A caller's table as the path files compare it: f32, the oracle's window rounded once; f64, the plan's own."""
    if dt == "f32":
        import oracle
        return torch.from_numpy(oracle.create_window(kind, n).astype(np.float32)).to(DEV)
    import test_gpu_f64_paths as F64
    return torch.from_numpy(F64.plan_window(n, kind)).to(DEV)


def build_spectrum(r):
    from pragma_dsp_amd.batch import BatchedFft
    import test_gpu_f32_paths as F32
    n, rows = r.shape
    p = BatchedFft(n, DEV, _t(r.dt))
    sides = "two" if r.op == "two" else "one"
    bins = n if sides == "two" else n // 2 + 1
    both = r.op == "amp-phase-peak"
    window, ref_window = "rect", None
    if r.op == "named":
        window, ref_window = "hann", ("plan", "hann")
    elif r.op == "table":
        window, ref_window = _table_window(r.dt, n, "hamming"), ("table", "hamming")
    state = {}

    def make(seed):
        frames, _ = F32.make_rows(np.random.default_rng([n, rows, seed, 2]), rows, n, False, first=seed)
        if seed == 0:
            state["frames"] = frames
        return [frames]

    ins = [torch.empty((rows, n), dtype=_t(r.dt), device=DEV)]
    outs = [torch.empty((rows, bins), dtype=_t(r.dt), device=DEV)]  # the amplitude rows: the API's only out=

    def call():
        return [t for t in p.spectrum(ins[0], window, sides, want_phase=both, want_peak=both, out=outs[0])
                if t is not None]

    def info_of(outputs):
        ph, pk = (outputs[1].data_ptr(), outputs[2].data_ptr()) if both else (None, None)
        wptr = None if r.op not in ("named", "table") else \
            (p.window("hann").data_ptr() if r.op == "named" else window.data_ptr())
        return path_info(r.dt, True, p._h, rows, ins[0].data_ptr(), n, n, wptr, int(sides == "two"),
                         outs[0].data_ptr(), ph, pk, None, 1.0)

    def check(eager):
        out = _spectrum_outputs(eager[0], eager[1] if both else None, eager[2] if both else None)
        if r.dt == "f32":
            out["path"] = F32.path_names(info_of(eager), n, spectrum=True)
        _check_spectrum(r, n, state["frames"], out, ref_window, sides)

    def guard(outputs):
        info = info_of(outputs)
        assert info[PATH] in SINGLE_PASS_SPECTRUM and info[PAIRS] == 0, info
        if n == 16384:  # the fused cosine-sum form of spectrum_dif16k_kernel
            assert info[PATH] == 14 and info[WMODE] in (2, 3), info

    return SimpleNamespace(ins=ins, make=make, outs=outs, call=call, check=check, guard=guard, keep=(p, window))


def build_peaks(r):
    from pragma_dsp_amd.batch import BatchedFft
    import test_gpu_f32_paths as F32
    n, rows = r.shape
    p = BatchedFft(n, DEV, torch.float32)
    state = {}

    def make(seed):
        frames, _ = F32.make_rows(np.random.default_rng([n, rows, seed, 3]), rows, n, False, first=seed)
        if seed == 0:
            state["frames"] = frames
        return [frames]

    ins = [torch.empty((rows, n), dtype=torch.float32, device=DEV)]

    def call():  # no out=: index, frequency, amplitude and phase of the records (views of one tensor), amp, phase
        return list(p.spectrum_peaks(ins[0], "rect", "one", sample_rate=F32.SR, want_amp=True, want_phase=True))

    def info_of(outputs):
        return path_info("f32", True, p._h, rows, ins[0].data_ptr(), n, n, None, 0, outputs[4].data_ptr(),
                         outputs[5].data_ptr(), None, outputs[0].data_ptr(), F32.SR)

    def check(eager):
        idx, freq, amp_at, ph_at, amp, ph = (t.cpu().numpy() for t in eager)
        rec = np.stack([idx] + [v.view(np.int32) for v in (freq, amp_at, ph_at)], axis=1)
        out = {"amp": amp, "ph": ph, "rec": np.ascontiguousarray(rec),
               "path": F32.path_names(info_of(eager), n, spectrum=True)}
        _check_spectrum(r, n, state["frames"], out, None, "one")

    def guard(outputs):
        info = info_of(outputs)
        # amplitude and phase rows are the caller's: peak_rows_extra is 0 whether or not the peaks are fused
        assert info[PATH] in SINGLE_PASS_SPECTRUM and info[PAIRS] == 0, info

    return SimpleNamespace(ins=ins, make=make, outs=[], call=call, check=check, guard=guard, keep=p)


def _hop(n, rows):
    return n // 4


def build_stft(r):
    from pragma_dsp_amd.batch import BatchedFft
    import test_gpu_f32_paths as F32
    import test_gpu_stft_pair as SP
    n, frames = r.shape
    hop = _hop(n, frames)
    length = n + (frames - 1) * hop
    p = BatchedFft(n, DEV, _t(r.dt))
    state = {}

    def make(seed):
        x = rounded(np.random.default_rng([n, frames, seed, 4]).standard_normal(length), "f32")
        if seed == 0:
            state["x"] = x
        return [x]

    ins = [torch.empty(length, dtype=_t(r.dt), device=DEV)]
    if r.op == "amp":
        call = lambda: [p.stft(ins[0], hop, "hann")[0]]  # noqa: E731
    else:
        call = lambda: list(p.stft_complex(ins[0], hop, "hann"))  # noqa: E731

    def info_of(outputs):
        return path_info(r.dt, True, p._h, frames, ins[0].data_ptr(), n, hop, p.window("hann").data_ptr(), 0,
                         outputs[0].data_ptr(), None, None, None, 1.0)

    def check(eager):
        x = state["x"]
        if r.op == "amp":
            idx = np.arange(frames)[:, None] * hop + np.arange(n)[None, :]
            out = {"amp": eager[0].cpu().numpy()}
            if r.dt == "f32":
                out["path"] = F32.path_names(info_of(eager), n, spectrum=True)
            _check_spectrum(r, n, x[idx], out, ("plan", "hann"), "one")
            return
        want = SP.ref_stft(x, n, hop, SP.win64(p, "hann"))
        got = SP.to_np(eager[0]) + 1j * SP.to_np(eager[1])
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"CAPTURE {r.name}: eager error {err:.3e}, bound {SP.FWD_TOL[_t(r.dt)] * math.log2(n):.3e}")
        assert err <= SP.FWD_TOL[_t(r.dt)] * math.log2(n), (r.name, err)

    def guard(outputs):
        if r.op == "amp":
            info = info_of(outputs)
            assert info[PATH] in SINGLE_PASS_SPECTRUM and info[PAIRS] == 0, info

    return SimpleNamespace(ins=ins, make=make, outs=[], call=call, check=check, guard=guard, keep=p)


def build_istft(r):
    from pragma_dsp_amd.batch import BatchedFft
    import test_gpu_stft_pair as SP
    import test_gpu_stft_paths as ST
    n, frames = r.shape
    hop = n  # the single-launch form; hop < N draws stream-ordered scratch (graph_capture_cases.EXCLUDED_FORMS)
    bins = n // 2 + 1
    p = BatchedFft(n, DEV, _t(r.dt))
    state = {}

    def make(seed):
        rng = np.random.default_rng([n, frames, seed, 5])
        re, im = (rounded(rng.standard_normal((frames, bins)), r.dt) for _ in range(2))
        if seed == 0:
            state["z"] = re + 1j * im
        return [re, im]

    ins = [torch.empty((frames, bins), dtype=_t(r.dt), device=DEV) for _ in range(2)]
    outs = [torch.empty(frames * n, dtype=_t(r.dt), device=DEV)]
    call = lambda: [p.istft(ins[0], ins[1], hop, "hann", out=outs[0])]  # noqa: E731

    def check(eager):
        want, den, ymax = SP.ref_istft(state["z"], n, hop, SP.win64(p, "hann"))
        got = SP.to_np(eager[0])
        assert ST.zeros_where_den_small(got, den)
        err = ST.inv_err(got, want, den, ymax, n, hop)
        print(f"CAPTURE {r.name}: eager error {err:.3e}, bound {SP.INV_TOL[_t(r.dt)] * math.log2(n):.3e}")
        assert err <= SP.INV_TOL[_t(r.dt)] * math.log2(n), (r.name, err)

    return SimpleNamespace(ins=ins, make=make, outs=outs, call=call, check=check, guard=lambda o: None, keep=p)


def build_dct(r):
    from pragma_dsp_amd.batch import BatchedFft
    import test_gpu_dct as TD
    from test_dct_cpu import dct_ref, idct_ref
    n, rows = r.shape
    name, t, layout = r.op
    norm = "ortho"
    p = BatchedFft(n, DEV, _t(r.dt))
    if layout == "fast":
        x = torch.empty((rows, n), dtype=_t(r.dt), device=DEV)
        y = torch.empty_like(x)
    else:  # a one-element offset: rows that are not 16-byte aligned take the general loads and stores
        xb, x = TD.strided(rows, n, n, r.dt, offset=1)
        yb, y = TD.strided(rows, n, n, r.dt, offset=1)
    assert TD._fast(x, y) == (layout == "fast")
    state = {}

    def make(seed):
        a = rounded(np.random.default_rng([n, rows, seed, 6]).standard_normal((rows, n)), r.dt)
        if seed == 0:
            state["x"] = a
        return [a]

    call = lambda: [getattr(p, name)(x, type=t, norm=norm, out=y)]  # noqa: E731

    def check(eager):
        want = (idct_ref if name == "idct" else dct_ref)(state["x"], t, norm)
        e = TD.rel_rows(eager[0].cpu().numpy(), want)
        lim = TD.TOL[r.dt] * (n.bit_length() - 1)
        print(f"CAPTURE {r.name}: eager error {e:.3e}, bound {lim:.3e}")
        assert e <= lim, (r.name, e)

    return SimpleNamespace(ins=[x], make=make, outs=[y], call=call, check=check, guard=lambda o: None, keep=p)


def build_hilbert(r):
    from pragma_dsp_amd.batch import BatchedFft
    import test_gpu_hilbert as TH
    from test_hilbert_cpu import hilbert_ref
    n, rows = r.shape
    mode = r.op
    p = BatchedFft(n, DEV, _t(r.dt))
    x = torch.empty((rows, n), dtype=_t(r.dt), device=DEV)
    odt = _t(r.dt) if mode != "analytic" else (torch.complex64 if r.dt == "f32" else torch.complex128)
    y = torch.empty((rows, n), dtype=odt, device=DEV)
    state = {}

    def make(seed):
        a = rounded(np.random.default_rng([n, rows, seed, 7]).standard_normal((rows, n)), r.dt)
        if seed == 0:
            state["x"] = a
        return [a]

    call = lambda: [TH.run(p, x, mode, out=y)]  # noqa: E731

    def check(eager):
        e = TH.err_rows(TH.to_np(eager[0]), hilbert_ref(state["x"]), mode)
        print(f"CAPTURE {r.name}: eager error {e:.3e}, bound {TH.bound(r.dt, n, mode):.3e}")
        assert e <= TH.bound(r.dt, n, mode), (r.name, e)

    return SimpleNamespace(ins=[x], make=make, outs=[y], call=call, check=check, guard=lambda o: None, keep=p)


def build_fir(r):
    import pragma_dsp_amd as pd
    from pragma_dsp_amd import _capi, _device, filters
    import test_gpu_fir_paths as TF
    n, rows = r.shape
    ntaps, length = G.FIR[n]
    if r.op == "spectrum":
        ntaps = G.fir_spectrum_taps(n)
    h0 = rounded(np.random.default_rng([n, 8]).standard_normal(ntaps), "f32")  # the same values in both precisions
    f = pd.FirFilter(h0, DEV, _t(r.dt), block=n)
    torch.cuda.synchronize()
    state = {}
    if r.op == "apply":
        x = torch.empty((rows, length), dtype=_t(r.dt), device=DEV)
        y = torch.empty((rows, length + ntaps - 1), dtype=_t(r.dt), device=DEV)

        def make(seed):
            a = rounded(np.random.default_rng([n, rows, seed, 9]).standard_normal((rows, length)), r.dt)
            if seed == 0:
                state["x"] = a
            return [a]

        call = lambda: [f.apply(x, "full", out=y)]  # noqa: E731

        def check(eager):
            e = TF.err(eager[0].cpu().numpy(), TF.f64_full(state["x"], h0), state["x"], h0)
            lim = TF.tol(r.dt, n, TF.TOL_GAUSS)
            print(f"CAPTURE {r.name}: eager error {e:.3e}, bound {lim:.3e}")
            assert e <= lim, (r.name, e)
            # H's launch has completed: the event that ordered apply() behind it is gone, a call is its kernel alone
            assert f._ready is None

        return SimpleNamespace(ins=[x], make=make, outs=[y], call=call, check=check, guard=lambda o: None, keep=f)

    # the filter's spectrum: FirFilter makes this very call once, in its constructor, on the taps it uploads there; the
    # capturable form is the call itself on device taps, with the filter's plan
    taps = torch.empty(ntaps, dtype=_t(r.dt), device=DEV)
    h_re, h_im = (torch.empty(n // 2 + 1, dtype=_t(r.dt), device=DEV) for _ in range(2))

    def make(seed):
        h = rounded(np.random.default_rng([n, seed, 10]).standard_normal(ntaps), "f32")
        if seed == 0:
            state["h"] = h
        return [h]

    def call():
        fn = getattr(filters.lib, f"pdsp_fir_spectrum_{r.dt}")
        _capi.check(fn(f.plan._h, _device.ptr(taps), ntaps, _device.ptr(h_re), _device.ptr(h_im),
                       _device.stream_ptr(f.device)))
        return [h_re, h_im]

    def check(eager):  # the bound of test_gpu_fir_paths.test_frequency_response_to_the_rounding
        h = state["h"]
        l1 = np.abs(h).sum()
        for got, ex in zip((t.cpu().numpy() for t in eager), TF.exact_dft(h, n)):
            d = np.abs(got.astype(np.longdouble) - ex).astype(np.float64)
            if r.dt == "f32":
                ulp = np.spacing(np.abs(ex.astype(np.float64)).astype(np.float32)).astype(np.float64)
                assert (d <= ulp + 2.0 ** -40 * l1).all(), (r.name, float((d / (ulp + 2.0 ** -40 * l1)).max()))
            else:
                assert d.max() <= TF.SPEC_TOL_F64[n] * l1, (r.name, d.max() / l1)

    return SimpleNamespace(ins=[taps], make=make, outs=[h_re, h_im], call=call, check=check, guard=lambda o: None,
                           keep=f)


def _complex_rows(seed, rows, ln, dt):
    rng = np.random.default_rng(seed)
    return rounded(rng.standard_normal((rows, ln)), dt), rounded(rng.standard_normal((rows, ln)), dt)


def build_dft(r):
    import pragma_dsp_amd as pd
    import test_gpu_dft as TDF
    ln, rows = r.shape
    d = pd.Dft(ln, DEV)
    ins = [torch.empty((rows, ln), dtype=_t(r.dt), device=DEV) for _ in range(2)]
    outs = [torch.empty((rows, ln), dtype=_t(r.dt), device=DEV) for _ in range(2)]
    state = {}

    def make(seed):
        re, im = _complex_rows([ln, rows, seed, 11], rows, ln, r.dt)
        if seed == 0:
            state["z"] = re + 1j * im
        return [re, im]

    call = lambda: list(getattr(d, r.op)(ins[0], ins[1], out=tuple(outs)))  # noqa: E731

    def check(eager):
        want = (np.fft.ifft if r.op == "inverse" else np.fft.fft)(state["z"])
        e = TDF.row_err(TDF.cplx(eager), want)
        print(f"CAPTURE {r.name}: eager error {e:.3e}, bound {TDF.bound(r.dt, ln):.3e}")
        assert e <= TDF.bound(r.dt, ln), (r.name, e)

    return SimpleNamespace(ins=ins, make=make, outs=outs, call=call, check=check, guard=lambda o: None, keep=d)


def build_czt(r):
    import pragma_dsp_amd as pd
    import test_gpu_czt as TC
    from test_czt_cpu import GRID, grid_direct, row_err
    ln, bins, rows = r.shape
    c = pd.Czt(ln, bins, TC.P / GRID, TC.Q / GRID, 1.0, DEV)  # a band of the circle: the zoom FFT's transform
    ins = [torch.empty((rows, ln), dtype=_t(r.dt), device=DEV) for _ in range(2)]
    outs = [torch.empty((rows, bins), dtype=_t(r.dt), device=DEV) for _ in range(2)]
    state = {}

    def make(seed):
        re, im = _complex_rows([ln, bins, seed, 12], rows, ln, r.dt)
        if seed == 0:
            state["z"] = re + 1j * im
        return [re, im]

    call = lambda: list(c.forward(ins[0], ins[1], out=tuple(outs)))  # noqa: E731

    def check(eager):
        z = state["z"]
        want = grid_direct(z, bins, TC.P, TC.Q, 1.0, extended=(r.dt == "f64"))
        e = row_err(TC.cplx(eager), want, z, 1.0)
        print(f"CAPTURE {r.name}: eager error {e:.3e}, bound {TC.bound(r.dt, ln, bins):.3e}")
        assert e <= TC.bound(r.dt, ln, bins), (r.name, e)

    return SimpleNamespace(ins=ins, make=make, outs=outs, call=call, check=check, guard=lambda o: None, keep=c)


def build_resample(r):
    import pragma_dsp_amd as pd
    import test_gpu_resample as TR
    from test_resample_cpu import user_taps
    if r.op == "poly":
        up, down, length, rows = r.shape
        h = pd.Resampler(up, down, device=DEV, dtype=_t(r.dt))
    else:
        up, down, ntaps, length, rows = r.shape
        h = pd.Upfirdn(user_taps(ntaps), up, down, device=DEV, dtype=_t(r.dt))
    x = torch.empty((rows, length), dtype=_t(r.dt), device=DEV)
    y = torch.empty((rows, h.output_len(length)), dtype=_t(r.dt), device=DEV)
    state = {}

    def make(seed):
        a = TR.signal((rows, length), _t(r.dt), 100 + seed)
        if seed == 0:
            state["x"] = a
        return [a]

    call = lambda: [h.apply(x, out=y)]  # noqa: E731

    def check(eager):
        # the family's check runs the handle on the same rows and holds every output to its bound; the eager result
        # kept from step 1 is that result bit for bit
        again = TR.check(h, state["x"], _t(r.dt), f"CAPTURE {r.name}")
        assert same_bits(again, eager[0])

    return SimpleNamespace(ins=[x], make=make, outs=[y], call=call, check=check, guard=lambda o: None, keep=h)


def build_dwt(r):
    import pragma_dsp_amd as pd
    import test_gpu_dwt as TW
    key, levels, n, rows = r.shape
    w = pd.Dwt(TW.wavelet(key), levels, DEV, _t(r.dt))
    assert levels > 1
    cs = TW.case(n, levels, key, _t(r.dt), rows)  # inputs and references, shared with the family's own tests
    x = torch.empty((rows, n), dtype=_t(r.dt), device=DEV)
    y = torch.empty_like(x)
    src, ref, lim = ("x", "fwd", "fwd_bound") if r.op == "forward" else ("c", "inv", "inv_bound")

    def make(seed):
        return [cs[src] if seed == 0 else TW.signal((rows, n), _t(r.dt), 1000 + n)]

    call = lambda: [getattr(w, r.op)(x, out=y)]  # noqa: E731

    def check(eager):
        TW.hold(TW.host(eager[0]), cs[ref], cs[lim], f"CAPTURE {r.name}")

    return SimpleNamespace(ins=[x], make=make, outs=[y], call=call, check=check, guard=lambda o: None, keep=w)


def build_ntt(r):
    import ntt_ref
    import pragma_dsp_amd as pd
    import test_gpu_ntt as TN
    n, rows = r.shape
    state = {}

    def words(xs):
        return np.array(xs, dtype=np.uint64)

    if r.op == "mul":
        a, b, out = (torch.empty((rows, n), dtype=torch.uint64, device=DEV) for _ in range(3))

        def make(seed):
            xs, ys = ntt_ref.rows(n, rows, seed, seed), ntt_ref.rows(n, rows, seed + 2, seed + 7)
            if seed == 0:
                state["want"] = [[u * v % ntt_ref.P for u, v in zip(p, q)] for p, q in zip(xs, ys)]
            return [words(xs), words(ys)]

        call = lambda: [pd.ntt_mul(a, b, out=out)]  # noqa: E731
        check = lambda eager: _equal(TN.host(eager[0]), state["want"], r.name)  # noqa: E731
        return SimpleNamespace(ins=[a, b], make=make, outs=[out], call=call, check=check, guard=lambda o: None,
                               keep=None)

    plan = pd.Ntt(n, DEV)
    if r.op in ("forward", "inverse"):
        x, out = (torch.empty((rows, n), dtype=torch.uint64, device=DEV) for _ in range(2))

        def make(seed):
            xs = ntt_ref.rows(n, rows, seed, seed)
            if seed == 0:
                state["want"] = ntt_ref.transform_rows(xs, inverse=r.op == "inverse")
            return [words(xs)]

        call = lambda: [getattr(plan, r.op)(x, out=out)]  # noqa: E731
        ins = [x]
    else:  # the cyclic product: a and b together longer than N, so the sum wraps
        a_len, b_len = n - 3, n // 4 + 1
        a = torch.empty((rows, a_len), dtype=torch.uint64, device=DEV)
        b = torch.empty((rows, b_len), dtype=torch.uint64, device=DEV)
        out = torch.empty((rows, n), dtype=torch.uint64, device=DEV)

        def make(seed):
            xs = [row[:a_len] for row in ntt_ref.rows(n, rows, seed, seed)]
            ys = [row[:b_len] for row in ntt_ref.rows(n, rows, seed + 2, seed + 7)]
            if seed == 0:
                state["want"] = [ntt_ref.cyclic(p, q, n) for p, q in zip(xs, ys)]
            return [words(xs), words(ys)]

        call = lambda: [plan.convolve(a, b, out=out)]  # noqa: E731
        ins = [a, b]
    check = lambda eager: _equal(TN.host(eager[0]), state["want"], r.name)  # noqa: E731
    return SimpleNamespace(ins=ins, make=make, outs=[out], call=call, check=check, guard=lambda o: None, keep=plan)


def _equal(got, want, name):
    assert got == want, name  # the NTT is exact: equality of 64-bit integers


def build_sdft(r):
    import pragma_dsp_amd as pd
    import sdft_ref as R
    import test_gpu_sdft as TS
    n, bins, hop, samples, rows = r.shape
    win = "hann"
    s = pd.SlidingDft(n, bins, hop=hop, window=win, device=DEV)
    frames = R.frames_of(n, hop, samples)
    x = torch.empty((rows, samples), dtype=_t(r.dt), device=DEV)
    outs = [torch.empty((rows, len(bins), frames), dtype=_t(r.dt), device=DEV) for _ in range(2)]
    state = {}

    def make(seed):
        a = rounded(np.random.default_rng([n, samples, seed, 13]).standard_normal((rows, samples)), "f32")
        if seed == 0:
            state["x"] = a
        return [a]

    call = lambda: list(s.forward(x, out=tuple(outs)))  # noqa: E731

    def check(eager):
        a = state["x"]
        dre, dim = R.direct(a, n, bins, hop, win, np.arange(frames))
        e = R.err_units(TS.cplx(*eager), dre, dim, n, r.dt, np.abs(a).max())
        print(f"CAPTURE {r.name}: eager error {e:.3f} of the bound {R.BOUND[r.dt]:.2f} u sqrt(N) max|x|")
        assert e <= R.BOUND[r.dt], (r.name, e)

    return SimpleNamespace(ins=[x], make=make, outs=outs, call=call, check=check, guard=lambda o: None, keep=s)


def build_elementwise(r):
    from pragma_dsp_amd import batch as B
    import test_gpu_elementwise as TE
    rows, n = r.shape
    dt = _np(r.dt)
    state = {}
    a, out = (torch.empty((rows, n), dtype=_t(r.dt), device=DEV) for _ in range(2))
    if r.op == "apply_window":
        w = torch.empty(n, dtype=_t(r.dt), device=DEV)

        def make(seed):
            rng = np.random.default_rng([rows, n, seed, 14])
            state[seed] = TE.draw(rng, rows * n, dt).reshape(rows, n), TE.draw(rng, n, dt)
            return list(state[seed])

        call = lambda: [B.apply_window(a, w, out=out)]  # noqa: E731

        def check(eager):  # one correctly rounded product: the numpy product in the dtype, bit for bit
            x, win = state[0]
            ib = np.int32 if r.dt == "f32" else np.int64
            assert np.array_equal(eager[0].cpu().numpy().view(ib), (x * win).view(ib))

        return SimpleNamespace(ins=[a, w], make=make, outs=[out], call=call, check=check, guard=lambda o: None,
                               keep=None)
    b = torch.empty_like(a)

    def make(seed):
        rng = np.random.default_rng([rows, n, seed, 15])
        state[seed] = TE.draw(rng, rows * n, dt).reshape(rows, n), TE.draw(rng, rows * n, dt).reshape(rows, n)
        return list(state[seed])

    call = lambda: [getattr(B, r.op)(a, b, out=out)]  # noqa: E731
    check = lambda eager: TE.judge_polar(r.op, r.dt, "capture", eager[0].cpu().numpy(), *state[0])  # noqa: E731
    return SimpleNamespace(ins=[a, b], make=make, outs=[out], call=call, check=check, guard=lambda o: None, keep=None)


def build_complex(r):
    from pragma_dsp_amd import batch as B
    import test_gpu_elementwise as TE
    rows, n = r.shape
    op = r.op
    binary = op in TE.BINARY
    ins = [torch.empty((rows, n), dtype=torch.float32, device=DEV) for _ in range(4 if binary else 2)]
    outs = [torch.empty((rows, n), dtype=torch.float32, device=DEV) for _ in range(2)]
    state = {}

    def make(seed):
        rng = np.random.default_rng([rows, n, seed, 16])
        state[seed] = [TE.draw(rng, rows * n).reshape(rows, n) for _ in ins]
        return state[seed]

    a, o = (ins[0], ins[1]), tuple(outs)
    if binary:
        call = lambda: list(getattr(B, "complex_" + op)(a, (ins[2], ins[3]), out=o))  # noqa: E731
    elif op == "conj":
        call = lambda: list(B.complex_conj(a, out=o))  # noqa: E731
    elif op == "scale":
        call = lambda: list(B.complex_scale(a, TE.SCALARS["scale"][0], out=o))  # noqa: E731
    else:
        call = lambda: list(B.complex_mul_scalar(a, *TE.SCALARS["mulScalar"], out=o))  # noqa: E731

    def check(eager):
        planes = [p.reshape(-1) for p in state[0]]
        TE.judge(op, "capture", [t.reshape(-1) for t in eager], TE.reference(op, *planes))

    return SimpleNamespace(ins=ins, make=make, outs=outs, call=call, check=check, guard=lambda o: None, keep=None)


BUILD = {"fft": build_fft, "spectrum": build_spectrum, "peaks": build_peaks, "stft": build_stft, "istft": build_istft,
         "dct": build_dct, "hilbert": build_hilbert, "fir": build_fir, "dft": build_dft, "czt": build_czt,
         "resample": build_resample, "dwt": build_dwt, "ntt": build_ntt, "sdft": build_sdft,
         "elementwise": build_elementwise, "complex": build_complex}


# ---- the procedure ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", G.ROWS, ids=G.IDS)
def test_capture_and_replay(row, monkeypatch):
    from pragma_dsp_amd import _capi
    live = BUILD[row.family](row)
    a, b = live.make(0), live.make(1)

    # 1. eager on A (recorded) and on B
    load(live.ins, a)
    proxy = RecordingLib(_capi.lib)
    with monkeypatch.context() as m:
        for name in MODULES:
            m.setattr(importlib.import_module("pragma_dsp_amd." + name), "lib", proxy)
        first = live.call()
    torch.cuda.synchronize()
    reached = {n for n in proxy.names if n in STREAM_ENTRIES}
    assert reached == set(row.entries), (sorted(reached), row.entries)
    eager_a = clones(first)
    load(live.ins, b)
    eager_b = clones(live.call())
    torch.cuda.synchronize()
    assert not all(same_bits(x, y) for x, y in zip(eager_a, eager_b)), "A and B must give different outputs"

    # 2. the eager result is itself right
    live.check(eager_a)
    live.guard(first)

    # 3. capture on a side stream; nothing runs
    load(live.ins, a)
    fill_sentinel(live.outs)
    torch.cuda.synchronize()
    gc.collect()  # a handle of an earlier row that is still awaiting collection frees its tables here, not below
    before = _capi.live_resources()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side_stream()):
        got = live.call()
    torch.cuda.synchronize()
    assert len(got) == len(eager_a)
    mine = {t.data_ptr() for t in live.outs}
    for t in live.outs:
        assert holds_sentinel(t), "an output changed during the capture: work ran outside the captured stream"
    assert all(t.data_ptr() in mine for t in got[:len(live.outs)])

    # 4. replay on A
    fill_sentinel(got)
    g.replay()
    torch.cuda.synchronize()
    for i, (t, want) in enumerate(zip(got, eager_a)):
        assert same_bits(t, want), f"output {i}: the replay on A differs from the eager call"

    # 5. replay on B, 6. twice more
    load(live.ins, b)
    for again in range(3):
        fill_sentinel(got)
        g.replay()
        torch.cuda.synchronize()
        for i, (t, want) in enumerate(zip(got, eager_b)):
            assert same_bits(t, want), f"output {i}: replay {again + 1} on B differs from the eager call"
    assert _capi.live_resources() == before, "capture or replay uploaded, allocated or created something"
    del g


def test_every_row_has_a_builder():
    assert {r.family for r in G.ROWS} == set(BUILD)


# ---- the refusal: a lazy upload on a capturing stream ------------------------------------------------------------------

def _unwarmed(kind):
    """(handle, the call that would upload, an eager check for afterwards) of a fresh handle."""
    import pragma_dsp_amd as pd
    if kind == "resampler":
        import test_gpu_resample as TR
        h = pd.Resampler(3, 2, device=DEV, dtype=torch.float32)
        x = TR.signal((3, 300), torch.float32, 5)
        xd = TR.dev(x, torch.float32)
        return h, lambda: h.apply(xd), lambda: TR.check(h, x, torch.float32, "after the refusal")
    if kind == "dwt":
        import test_gpu_dwt as TW
        key, levels, n, rows = G.DWT
        h = pd.Dwt(key, levels, DEV, torch.float64)
        cs = TW.case(n, levels, key, torch.float64, rows)
        xd = TW.dev(cs["x"], torch.float64)
        return h, lambda: h.forward(xd), \
            lambda: TW.hold(TW.host(h.forward(xd)), cs["fwd"], cs["fwd_bound"], "after the refusal")
    if kind == "ntt":
        import ntt_ref
        import test_gpu_ntt as TN
        h = pd.Ntt(64, DEV)
        xs = ntt_ref.rows(64, 5)
        xd = TN.dev(xs)
        return h, lambda: h.forward(xd), lambda: _equal(TN.host(h.forward(xd)), ntt_ref.transform_rows(xs), "ntt")
    from pragma_dsp_amd.batch import BatchedFft
    import test_gpu_stft_pair as SP
    n, hop = 64, 16
    h = BatchedFft(n, DEV, torch.float32)
    x = rounded(np.random.default_rng(17).standard_normal(n + 4 * hop), "f32")
    xd = dev(x, "f32")

    def after():
        re, im = h.stft_complex(xd, hop, "hann")
        want = SP.ref_stft(x, n, hop, SP.win64(h, "hann"))
        err = np.abs(SP.to_np(re) + 1j * SP.to_np(im) - want).max() / np.abs(want).max()
        assert err <= SP.FWD_TOL[torch.float32] * math.log2(n)

    return h, lambda: h.stft_complex(xd, hop, "hann"), after


@pytest.mark.parametrize("kind", ["resampler", "dwt", "ntt", "window"])
def test_a_lazy_upload_on_a_capturing_stream_is_refused(kind):
    import pragma_dsp_amd as pd
    from pragma_dsp_amd import _capi
    from pragma_dsp_amd.batch import BatchedFft
    import test_gpu_f32_paths as F32
    # the warmed call of another handle that shares the capture
    n, rows = 64, 5
    warm = BatchedFft(n, DEV, torch.float32)
    re, im = F32.make_rows(np.random.default_rng(23), rows, n, True)
    dre, dim = dev(re, "f32"), dev(im, "f32")
    outs = [torch.empty_like(dre), torch.empty_like(dre)]
    warm.forward(dre, dim, out=tuple(outs))
    torch.cuda.synchronize()
    eager = clones(outs)
    handle, call, after = _unwarmed(kind)
    fill_sentinel(outs)
    torch.cuda.synchronize()
    gc.collect()
    before = _capi.live_resources()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side_stream()):
        warm.forward(dre, dim, out=tuple(outs))
        with pytest.raises(pd.PdspError) as e:
            call()
    # the capture ended normally: no HIP call that a capture forbids was made before the refusal
    assert str(e.value).startswith("stream is capturing:") and e.value.code == _capi.ERR_BAD_ARG, str(e.value)
    torch.cuda.synchronize()
    assert all(holds_sentinel(t) for t in outs)
    assert _capi.live_resources() == before, "the refused call left a table behind"
    g.replay()
    torch.cuda.synchronize()
    assert all(same_bits(t, want) for t, want in zip(outs, eager))
    del g
    # the handle is still usable: an eager call uploads the table and is right
    after()
    torch.cuda.synchronize()
    assert _capi.live_resources()["tables"] == before["tables"] + 1

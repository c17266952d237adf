"""The aliasing contract of the single-pass transforms and of the spectra (include/pdsp_hip.h), row by
row of tests/aliasing_cases.py: one row per (entry point, dtype, kernel reached).

Every row runs the same steps on one byte arena that holds the inputs, room of an output's size before and behind each
input, the window table and the disjoint outputs, all between bands of 0xFF bytes (NaN as a float, -1 as an int):
  1. the disjoint call, held to the reference and bound of test_gpu_f32_paths / test_gpu_f64_paths: the baseline;
  2. every admitted form, twice: the path query names the baseline's path, the outputs equal the baseline bit for bit
     and no byte outside them changes.  The comparison is with the disjoint call whose outputs have the form's
     alignment, which is the baseline itself unless the form moves an output to another alignment class;
  3. every refused form: PDSP_ERR_BAD_ARG and the exact text from the call and from the path query, no byte of the
     arena changed (nothing was launched), the counters of pdsp_dev_live_resources unchanged, and the next legal call
     on the plan equal to the baseline;
  4. adjacency: an output directly behind an input and directly in front of one is accepted and equals the baseline.
No test here runs a racing overlap on the device: the forms that would race are the refused ones, which launch nothing.

The kernel a row reaches is asserted on pdsp_dev_transform_path_* / pdsp_dev_spectrum_path_* and on the mirrors
expected_path / expected_path_f64 before every call (the interleaved entry points have one kernel and no query).
"""
import ctypes

import numpy as np
import pytest

import aliasing_cases as AC
import test_gpu_f32_paths as F32
import test_gpu_f64_paths as F64

pytestmark = pytest.mark.gpu

BAND = 4096   # bytes of 0xFF around and between the buffers
ALIGN = 256   # every region starts on a multiple of this, plus its row's misalignment
ERR_BAD_ARG = 9
TEXT_PLANAR = (b"output overlaps input (an output plane may share bytes with an input plane only where the two begin at "
               b"the same address)")
TEXT_PLANES = b"the output planes overlap each other"
TEXT_INTERLEAVED = b"output overlaps input (only out == in may share bytes)"
TEXT_SPECTRUM = b"output overlaps input (the spectrum has no in-place form)"
TEXT_OUTPUTS = b"the outputs overlap each other"


def _mod(dt):
    return F32 if dt == "f32" else F64


def _np(dt):
    return np.float32 if dt == "f32" else np.float64


def _lib():
    return F32._lib()


@pytest.fixture(scope="module", autouse=True)
def _plans():
    import torch
    F64.check_long_double()
    yield
    for m in (F32, F64):
        for p in m._PLANS.values():
            p.close()
        m._PLANS.clear()
    torch.cuda.empty_cache()


class Arena:
    """`size` bytes on the device, all 0xFF but what put() places.  Addresses are byte offsets."""

    def __init__(self, size):
        import torch
        self.t = torch.empty(size, dtype=torch.uint8, device="cuda:0")
        self.base = self.t.data_ptr()
        assert self.base % ALIGN == 0
        self.inputs = []

    def put(self, off, a):
        self.inputs.append((off, np.ascontiguousarray(a).view(np.uint8).reshape(-1)))

    def reset(self):
        import torch
        self.t.fill_(0xFF)
        for off, b in self.inputs:
            self.t[off:off + b.size].copy_(torch.from_numpy(b))

    def ptr(self, off):
        return self.base + off

    def snap(self):
        import torch
        torch.cuda.synchronize()
        return self.t.cpu().numpy()


class Layout:
    """Regions of an arena, laid out in order: name -> byte offset."""

    def __init__(self):
        self.at, self.end = {}, BAND

    def add(self, name, nbytes, misalign=0, room=0):
        start = -(-(self.end + room) // ALIGN) * ALIGN + misalign
        self.at[name] = start
        self.end = start + nbytes + room + BAND
        return start


def first_diff(got, want, dtype):
    """'element i: got 0x.., want 0x..' of the first differing element of two byte arrays."""
    es = np.dtype(dtype).itemsize
    g, w = got.view(f"u{es}"), want.view(f"u{es}")
    i = int(np.flatnonzero(g != w)[0])
    return f"element {i}: got {int(g[i]):#0{2 + 2 * es}x}, want {int(w[i]):#0{2 + 2 * es}x}"


def same_bits(got, want, dtype, ctx):
    assert np.array_equal(got, want), (ctx, first_diff(got, want, dtype))


def untouched(before, after, written, ctx):
    """No byte outside the `written` (offset, size) ranges differs."""
    mask = np.ones(before.size, bool)
    for off, size in written:
        mask[off:off + size] = False
    bad = np.flatnonzero((before != after) & mask)
    assert bad.size == 0, (ctx, f"byte {int(bad[0]) if bad.size else -1} outside the outputs changed")


def refused(call, query, text, arena, ctx):
    """Step 3 for one form: `call` and `query` return the status; nothing may happen."""
    from pragma_dsp_amd._capi import live_resources
    lib = _lib()
    live = live_resources()
    before = arena.snap()
    rc = call()
    assert (rc, lib.pdsp_last_error()) == (ERR_BAD_ARG, text), (ctx, "call", rc, lib.pdsp_last_error())
    if query is not None:
        rc = query()
        assert (rc, lib.pdsp_last_error()) == (ERR_BAD_ARG, text), (ctx, "path query", rc, lib.pdsp_last_error())
    after = arena.snap()
    assert np.array_equal(before, after), (ctx, "a refused call wrote", first_diff(after, before, np.uint8))
    assert live_resources() == live, (ctx, "a refused call changed the live resources")


# ---- transforms ---------------------------------------------------------------------------------------------------

class Planar:
    """One planar transform row: the arena with room of a plane before and behind each input plane."""

    def __init__(self, row, out_offs=None):
        self.row, self.m = row, _mod(row.dt)
        self.es = 4 if row.dt == "f32" else 8
        self.P = row.batch * row.n * self.es  # bytes of a plane
        offs = list(row.offs)
        if out_offs is not None:
            offs[2:] = out_offs
        lay = Layout()
        self.A = lay.add("A", self.P, offs[0] * self.es, room=self.P + ALIGN)
        self.B = lay.add("B", self.P, offs[1] * self.es, room=self.P + ALIGN) if row.kind != "real" else None
        self.C = lay.add("C", self.P, offs[2] * self.es)
        self.D = lay.add("D", self.P, offs[3] * self.es)
        self.arena = Arena(lay.end)
        self.plan = self.m.plan(row.n)
        fn = {"complex": "pdsp_fft_forward_complex_", "real": "pdsp_fft_forward_real_", "inverse": "pdsp_fft_inverse_"}
        self.fn = getattr(_lib(), fn[row.kind] + row.dt)
        self.qfn = getattr(_lib(), "pdsp_dev_transform_path_" + row.dt)

    def load(self, re, im):
        self.arena.put(self.A, re.astype(_np(self.row.dt)))
        if im is not None:
            self.arena.put(self.B, im.astype(_np(self.row.dt)))

    def _args(self, ro, io):
        a = self.arena
        ins = (a.ptr(self.A),) if self.B is None else (a.ptr(self.A), a.ptr(self.B))
        return (self.plan._h, self.row.batch) + ins + (a.ptr(ro), a.ptr(io))

    def call(self, ro, io):
        return self.fn(*self._args(ro, io), self.m._stream())

    def query(self, ro, io, info=None):
        args = self._args(ro, io)
        if self.B is None:
            args = args[:3] + (None,) + args[3:]
        info = info or (ctypes.c_int * F32.PATH_INFO)()
        return self.qfn(*args, 1 if self.row.kind == "inverse" else 0, info)

    def path(self, ro, io):
        """The library's answer for this call, in the mirror's names, and the mirror must agree."""
        row = self.row
        info = (ctypes.c_int * F32.PATH_INFO)(*([-1] * F32.PATH_INFO))
        assert self.query(ro, io, info) == 0, _lib().pdsp_last_error()
        names = (F32.path_names if row.dt == "f32" else F64.path_names_f64)(list(info), row.n)
        off = lambda b: None if b is None else (b % ALIGN) // self.es  # noqa: E731
        poffs = (off(self.A), off(self.B), off(ro), off(io))
        expected = F32.expected_path if row.dt == "f32" else F64.expected_path_f64
        mirror = expected(row.kind, row.n, row.batch, poffs, switches=row.switches)
        assert names == mirror, (row.name, poffs, sorted(names), sorted(mirror))
        return names

    def run(self, ro, io, ctx):
        """One accepted call from a fresh arena: (re bytes, im bytes, path names); nothing else may change."""
        a = self.arena
        a.reset()
        before = a.snap()
        names = self.path(ro, io)
        rc = self.call(ro, io)
        after = a.snap()
        assert rc == 0, (ctx, _lib().pdsp_last_error())
        untouched(before, after, [(ro, self.P), (io, self.P)], ctx)
        return after[ro:ro + self.P].copy(), after[io:io + self.P].copy(), names


def _planar_baseline(row, re, im, ref, out_offs, cache):
    """The disjoint call with output planes at these misalignments (None: the row's own), held to the family's bound."""
    key = tuple(o % 16 for o in (row.offs[2:] if out_offs is None else out_offs))
    if key not in cache:
        m, dtype = _mod(row.dt), _np(row.dt)
        t = Planar(row, key)
        t.load(re, im)
        bre, bim, names = t.run(t.C, t.D, (row.name, "disjoint", key))
        got = bre.view(dtype).reshape(row.batch, row.n).astype(np.float64) + \
            1j * bim.view(dtype).reshape(row.batch, row.n).astype(np.float64)
        kind = "inv" if row.kind == "inverse" else "fwd"
        errs = m.row_errors(got, ref)
        assert errs.max() <= m.bound(kind, row.n), (row.name, "disjoint", key, float(errs.max()) / m.lg(row.n))
        cache[key] = (bre, bim, names)
    return cache[key]


@pytest.mark.parametrize("row", [r for r in AC.TRANSFORM_ROWS if r.kind in AC.PLANAR],
                         ids=[r.name for r in AC.TRANSFORM_ROWS if r.kind in AC.PLANAR])
def test_planar_transform_aliasing(row):
    m, dtype = _mod(row.dt), _np(row.dt)
    rng = np.random.default_rng(sum(map(ord, row.name)))
    re, im = m.make_rows(rng, row.batch, row.n, row.kind != "real")
    ref = m.reference_transform(row.kind, re, im)
    cache = {}
    with F32.Switches(row.switches):
        base = _planar_baseline(row, re, im, ref, None, cache)
        assert row.kernel in base[2], (row.name, sorted(base[2]))
        t = Planar(row)
        t.load(re, im)
        A, B, C, D, P, es = t.A, t.B, t.C, t.D, t.P, t.es
        X = A if B is None else B  # the input plane the second output is tried against
        if B is None:
            admitted = {"re-in-place": (A, D), "im-over-re": (C, A)}
        else:
            admitted = {"in-place": (A, B), "exchanged": (B, A), "re-in-place": (A, D), "im-in-place": (C, B),
                        "re-over-im": (B, D), "im-over-re": (C, A)}
        # 4. adjacency: directly behind and directly in front of an input plane
        admitted.update({"re-behind-in": (A + P, D), "re-before-in": (A - P, D), "im-behind-in": (C, X + P),
                         "im-before-in": (C, X - P)})
        for form, (ro, io) in admitted.items():
            # the disjoint call whose output planes have this form's alignment: the baseline itself for most forms
            want = _planar_baseline(row, re, im, ref, ((ro % ALIGN) // es % 16, (io % ALIGN) // es % 16), cache)
            for turn in (1, 2):
                ctx = (row.name, form, turn)
                gre, gim, names = t.run(ro, io, ctx)
                assert names == want[2], (ctx, sorted(names), sorted(want[2]))
                # (an adjacent plane may sit in another alignment class -- N = 2: a plane of 4097 rows ends 8 bytes
                # off -- and run on another kernel: `want` is the disjoint call at that alignment)
                assert row.kernel in names or form.endswith("-in"), (ctx, sorted(names))
                same_bits(gre, want[0], dtype, ctx + ("re",))
                same_bits(gim, want[1], dtype, ctx + ("im",))
        # 3. refused forms
        row_b, half = row.n * es, (row.batch * row.n // 2) * es
        forms = []
        for shift, tag in ((es, "one-element"), (row_b, "one-row"), (half, "half-a-plane"), (1 - P, "last-byte-on-first")):
            forms.append((f"re_out {tag} into re_in", A + shift, D, TEXT_PLANAR))
            forms.append((f"im_out {tag} into {'re_in' if B is None else 'im_in'}", C, X + shift, TEXT_PLANAR))
        forms.append(("im_out one element into re_out", C, C + es, TEXT_PLANES))
        forms.append(("im_out one row into re_out", C, C + row_b, TEXT_PLANES))
        t.arena.reset()
        for form, ro, io, text in forms:
            ctx = (row.name, form)
            refused(lambda: t.call(ro, io), lambda: t.query(ro, io), text, t.arena, ctx)
            gre, gim, _ = t.run(C, D, ctx + ("the next legal call",))
            same_bits(gre, base[0], dtype, ctx + ("next call, re",))
            same_bits(gim, base[1], dtype, ctx + ("next call, im",))


@pytest.mark.parametrize("row", [r for r in AC.TRANSFORM_ROWS if r.kind not in AC.PLANAR],
                         ids=[r.name for r in AC.TRANSFORM_ROWS if r.kind not in AC.PLANAR])
def test_interleaved_transform_aliasing(row):
    m, dtype = _mod(row.dt), _np(row.dt)
    es = np.dtype(dtype).itemsize
    rng = np.random.default_rng(sum(map(ord, row.name)))
    re, im = m.make_rows(rng, row.batch, row.n, True)
    ref = m.reference_transform(row.kind, re, im)
    z = np.empty((row.batch, 2 * row.n), dtype)
    z[:, 0::2], z[:, 1::2] = re, im
    P = z.nbytes
    lay = Layout()
    IN = lay.add("in", P, room=P + ALIGN)
    OUT = lay.add("out", P)
    a = Arena(lay.end)
    a.put(IN, z)
    plan = m.plan(row.n)
    fn = getattr(_lib(), row.entry)
    expected = F32.expected_path if row.dt == "f32" else F64.expected_path_f64
    assert expected(row.kind, row.n, row.batch, (0, 0, 0, 0)) == {row.kernel}

    def call(out):
        return fn(plan._h, row.batch, a.ptr(IN), a.ptr(out), m._stream())

    def run(out, ctx):
        a.reset()
        before = a.snap()
        rc = call(out)
        after = a.snap()
        assert rc == 0, (ctx, _lib().pdsp_last_error())
        untouched(before, after, [(out, P)], ctx)
        return after[out:out + P].copy()

    base = run(OUT, (row.name, "disjoint"))
    g = base.view(dtype).reshape(row.batch, 2 * row.n).astype(np.float64)
    errs = m.row_errors(g[:, 0::2] + 1j * g[:, 1::2], ref)
    kind = "inv" if row.kind == "iinv" else "fwd"
    assert errs.max() <= m.bound(kind, row.n), (row.name, "disjoint", float(errs.max()) / m.lg(row.n))
    for form, out in (("in-place", IN), ("behind-in", IN + P), ("before-in", IN - P)):
        for turn in (1, 2):
            same_bits(run(out, (row.name, form, turn)), base, dtype, (row.name, form, turn))
    pair, row_b = 2 * es, 2 * row.n * es
    half = (row.batch * row.n // 2) * pair
    a.reset()
    for form, shift in (("one pair", pair), ("one row", row_b), ("half the rows", half), ("last pair on first", pair - P)):
        ctx = (row.name, f"out {form} into in")
        refused(lambda: call(IN + shift), None, TEXT_INTERLEAVED, a, ctx)
        same_bits(run(OUT, ctx + ("the next legal call",)), base, dtype, ctx + ("next call",))


# ---- spectra ------------------------------------------------------------------------------------------------------

class Spectrum:
    """One spectrum row: frames (or the signal of overlapping frames) with room of the largest output before and
    behind, the window table, and the outputs the row asks for."""

    def __init__(self, row, frames, signal):
        import oracle
        self.row, self.m = row, _mod(row.dt)
        dtype = _np(row.dt)
        self.es = es = np.dtype(dtype).itemsize
        n, batch = row.n, row.batch
        self.bins = n // 2 + 1 if row.sides == "one" else n
        self.size = {"amp": batch * self.bins * es, "ph": batch * self.bins * es, "idx": batch * 4, "rec": batch * 16}
        self.ext = ((batch - 1) * row.stride + n) * es  # the frames' extent in bytes
        room = max(self.size[k] for k in row.outputs) + ALIGN
        lay = Layout()
        self.FR = lay.add("frames", self.ext, room=room)
        self.W = lay.add("window", n * es) if row.window and row.window[0] == "table" else None
        self.out = {k: lay.add(k, self.size[k]) for k in ("amp", "ph", "idx", "rec") if k in row.outputs}
        self.arena = Arena(lay.end)
        self.arena.put(self.FR, (signal if signal is not None else frames).astype(dtype))
        self.plan = self.m.plan(n)
        self.wptr = None
        if row.window and row.window[0] == "plan":
            self.wptr = self.plan.window(row.window[1]).data_ptr()
        elif row.window and row.dt == "f32":
            self.arena.put(self.W, oracle.create_window(row.window[1], n).astype(np.float32))
        elif row.window:
            self.arena.put(self.W, F64.plan_window(n, row.window[1]))
        if self.W is not None:
            self.wptr = self.arena.ptr(self.W)
        self.qfn = getattr(_lib(), "pdsp_dev_spectrum_path_" + row.dt)

    def _ptrs(self, at):
        return [self.arena.ptr(at[k]) if k in at else None for k in ("amp", "ph", "idx", "rec")]

    def call(self, at):
        row, lib = self.row, _lib()
        amp, ph, idx, rec = self._ptrs(at)
        head = (self.plan._h, row.batch, self.arena.ptr(self.FR), row.n, row.stride, self.wptr,
                1 if row.sides == "two" else 0)
        if row.entry == AC.SP:
            return lib.pdsp_spectrum_peaks_f32(*head, F32.SR, amp, ph, rec, self.m._stream())
        return getattr(lib, row.entry)(*head, amp, ph, idx, self.m._stream())

    def query(self, at, info=None):
        row = self.row
        info = info or (ctypes.c_int * F32.PATH_INFO)()
        return self.qfn(self.plan._h, row.batch, self.arena.ptr(self.FR), row.n, row.stride, self.wptr,
                        1 if row.sides == "two" else 0, *self._ptrs(at), F32.SR if "rec" in at else 1.0, info)

    def path(self, at):
        row = self.row
        info = (ctypes.c_int * F32.PATH_INFO)(*([-1] * F32.PATH_INFO))
        assert self.query(at, info) == 0, _lib().pdsp_last_error()
        names = (F32.path_names if row.dt == "f32" else F64.path_names_f64)(list(info), row.n, spectrum=True)
        expected = F32.expected_path if row.dt == "f32" else F64.expected_path_f64
        mirror = expected("spectrum", row.n, row.batch, (0, 0 if row.window else None), frame_len=row.n,
                          stride=row.stride, window=row.window, sides=row.sides, outputs=set(row.outputs))
        assert names == mirror, (row.name, sorted(names), sorted(mirror))
        return names

    def run(self, at, ctx):
        a = self.arena
        a.reset()
        before = a.snap()
        names = self.path(at)
        rc = self.call(at)
        after = a.snap()
        assert rc == 0, (ctx, _lib().pdsp_last_error())
        untouched(before, after, [(at[k], self.size[k]) for k in at], ctx)
        return {k: after[at[k]:at[k] + self.size[k]].copy() for k in at}, names


@pytest.mark.parametrize("row", AC.SPECTRUM_ROWS, ids=[r.name for r in AC.SPECTRUM_ROWS])
def test_spectrum_aliasing(row):
    m, dtype = _mod(row.dt), _np(row.dt)
    rng = np.random.default_rng(sum(map(ord, row.name)))
    if row.stride < row.n:
        frames, signal = m.spectrum_rows(rng, row.batch, row.n, row.n, row.stride, "hop", 0)
    else:
        frames, signal = m.make_rows(rng, row.batch, row.n, False)[0], None
    s = Spectrum(row, frames, signal)
    es, FR = s.es, s.FR
    base, names = s.run(s.out, (row.name, "disjoint"))
    assert any(p.startswith(row.kernel) for p in names), (row.name, sorted(names))
    if "rec" in row.outputs:
        assert {"peak_wave_kernel"} <= names or any(p.endswith("-peak") for p in names), sorted(names)
    out = {"path": names}
    for k, b in base.items():
        out[k] = b.view(dtype).reshape(row.batch, s.bins) if k in ("amp", "ph") else \
            b.view(np.int32).reshape(row.batch, -1)
    fails = m.check_spectrum(F32.Worst(lambda *a: None, row.name), row.n, frames, out, row.window, row.sides, row.name)
    assert not fails, fails

    def same(got, ctx):
        for k in base:
            same_bits(got[k], base[k], dtype if k in ("amp", "ph") else np.int32, ctx + (k,))

    # 4. adjacency: the first output directly behind the frames' extent, and directly in front of the frames
    first = row.outputs[0]
    for form, at in (("behind the frames", FR + s.ext), ("before the frames", FR - s.size[first])):
        ctx = (row.name, f"{first} directly {form}")
        got, path = s.run(dict(s.out, **{first: at}), ctx)
        assert path == names, (ctx, sorted(path))
        same(got, ctx)
    # 3. refused forms
    forms = []
    for k in row.outputs:
        shifts = [("one element into", es), ("one row into", row.stride * es), ("half way into", s.ext // (2 * es) * es),
                  ("with its last byte on the first of", 1 - s.size[k]), ("on the last sample of", s.ext - es)]
        forms += [(f"{k} {tag} the frames", dict(s.out, **{k: FR + sh}), TEXT_SPECTRUM) for tag, sh in shifts]
        if s.wptr is not None:  # the caller's table in the arena, or the plan's own table (an address, never written)
            forms.append((f"{k} inside the window", dict(s.out, **{k: s.wptr + 4 * es - s.arena.base}), TEXT_SPECTRUM))
    if len(row.outputs) > 1 and "amp" in row.outputs:
        k = [o for o in row.outputs if o != "amp"][0]
        forms.append((f"{k} one element into amp", dict(s.out, **{k: s.out["amp"] + es}), TEXT_OUTPUTS))
        forms.append((f"{k} one row into amp", dict(s.out, **{k: s.out["amp"] + s.bins * es}), TEXT_OUTPUTS))
    if "rec" in row.outputs and "amp" in row.outputs:
        forms.append(("peak records inside amp", dict(s.out, rec=s.out["amp"] + 16), TEXT_OUTPUTS))
    s.arena.reset()
    for form, at, text in forms:
        ctx = (row.name, form)
        refused(lambda: s.call(at), lambda: s.query(at), text, s.arena, ctx)
        got, _ = s.run(s.out, ctx + ("the next legal call",))
        same(got, ctx + ("next call",))


# ---- multi-pass sizes keep every in / out overlap -----------------------------------------------------------------

@pytest.mark.parametrize("dt,n", [("f32", 1 << 15), ("f64", 1 << 14)], ids=["f32-2p15", "f64-2p14"])
def test_multi_pass_sizes_keep_their_overlaps(dt, n):
    """Beyond the single-pass limit the first pass reads the input into planes of its own: in place and an output half
    a plane into the input are accepted and held to the bound, as before.  Output planes that overlap each other are
    refused there too."""
    m = _mod(dt)
    row = AC.TRow(f"multi-pass-{dt}", f"pdsp_fft_forward_complex_{dt}", "complex", dt, n, 2, (0, 0, 0, 0), None, None)
    rng = np.random.default_rng(n)
    re, im = m.make_rows(rng, row.batch, n, True)
    ref = m.reference_transform("complex", re, im)
    dtype = _np(dt)
    t = Planar(row)
    t.load(re, im)
    half = t.P // 2
    for form, ro, io in (("disjoint", t.C, t.D), ("in-place", t.A, t.B), ("half a plane into re_in", t.A + half, t.D),
                         ("half a plane into im_in", t.C, t.B + half)):
        a = t.arena
        a.reset()
        before = a.snap()
        info = (ctypes.c_int * F32.PATH_INFO)()
        assert t.query(ro, io, info) == 0, (form, _lib().pdsp_last_error())
        assert t.call(ro, io) == 0, (form, _lib().pdsp_last_error())
        after = a.snap()
        # an input plane under an output is overwritten; the rest of the arena stays
        untouched(before, after, [(ro, t.P), (io, t.P)], (row.name, form))
        got = after[ro:ro + t.P].view(dtype).reshape(2, n).astype(np.float64) + \
            1j * after[io:io + t.P].view(dtype).reshape(2, n).astype(np.float64)
        errs = m.row_errors(got, ref)
        assert errs.max() <= m.bound("fwd", n), (row.name, form, float(errs.max()) / m.lg(n))
    t.arena.reset()
    for form, io in (("one element", t.C + t.es), ("one row", t.C + n * t.es)):
        refused(lambda: t.call(t.C, io), lambda: t.query(t.C, io), TEXT_PLANES, t.arena,
                (row.name, f"im_out {form} into re_out"))


# ---- in place where workgroups replace each other on a CU ---------------------------------------------------------

FULL = [("f32", 64, 64, "fft_staged_kernel"), ("f32", 4096, 1, "fft_stockham_kernel"),
        ("f64", 4096, 1, "fft_stockham_kernel"), ("f32", 16384, 1, "fft_split4_kernel")]


@pytest.mark.parametrize("dt,n,rows_per_wg,kernel", FULL, ids=[f"{c[0]}-{c[1]}" for c in FULL])
def test_in_place_at_a_machine_filling_grid(dt, n, rows_per_wg, kernel):
    """W = 32 x CUs workgroups (test_gpu_full_machine's W: a CU holds at most 32 workgroups, so later ones start where
    earlier ones retire) and a partial one more: the in-place call equals the disjoint call bit for bit.  Four planes
    of the batch: 0.5 GiB in f32, 1 GiB in f64 at N = 4096."""
    import torch
    import full_machine_cases as FM
    m = _mod(dt)
    lib = _lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    batch = FM.ROUNDS * cus * rows_per_wg + (rows_per_wg // 2 if rows_per_wg > 1 else 1)
    tdt = torch.float32 if dt == "f32" else torch.float64
    g = torch.Generator(device="cuda:0").manual_seed(n)
    re = torch.randn((batch, n), dtype=tdt, device="cuda:0", generator=g)
    im = torch.randn((batch, n), dtype=tdt, device="cuda:0", generator=g)
    ore, oim = torch.empty_like(re), torch.empty_like(im)
    p = m.plan(n)
    info = (ctypes.c_int * F32.PATH_INFO)(*([-1] * F32.PATH_INFO))
    q = getattr(lib, "pdsp_dev_transform_path_" + dt)
    names = F32.path_names if dt == "f32" else F64.path_names_f64
    fn = getattr(lib, "pdsp_fft_forward_complex_" + dt)
    for out in ((ore, oim), (re, im)):
        assert q(p._h, batch, re.data_ptr(), im.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), 0, info) == 0
        assert names(list(info), n) == {kernel}, sorted(names(list(info), n))
        assert fn(p._h, batch, re.data_ptr(), im.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), m._stream()) == 0, \
            lib.pdsp_last_error()
    torch.cuda.synchronize()
    bits = torch.int32 if dt == "f32" else torch.int64
    for name, got, want in (("re", re, ore), ("im", im, oim)):
        ne = (got.view(bits) != want.view(bits)).reshape(-1)
        if bool(ne.any()):
            i = int(torch.nonzero(ne)[0])
            raise AssertionError((dt, n, name, f"element {i} (row {i // n}): got "
                                  f"{int(got.view(bits).reshape(-1)[i]):#x}, want {int(want.view(bits).reshape(-1)[i]):#x}"))
    del re, im, ore, oim
    torch.cuda.empty_cache()


# ---- Python ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", AC.DTS)
def test_python_out_is_the_input(dt):
    """BatchedFft.forward / inverse / forward_interleaved with out= the inputs give the bits of a fresh output, and
    spectrum(out=) pointing into the frames raises."""
    import torch
    from pragma_dsp_amd._capi import PdspError, ERR_BAD_ARG as BAD
    m = _mod(dt)
    tdt = torch.float32 if dt == "f32" else torch.float64
    n, batch = 4096, 5
    p = m.plan(n)
    g = torch.Generator(device="cuda:0").manual_seed(7)
    re = torch.randn((batch, n), dtype=tdt, device="cuda:0", generator=g)
    im = torch.randn((batch, n), dtype=tdt, device="cuda:0", generator=g)
    bits = torch.int32 if dt == "f32" else torch.int64

    def eq(a, b):
        return bool((a.view(bits) == b.view(bits)).all())

    for name, fn in (("forward", p.forward), ("inverse", p.inverse)):
        fre, fim = fn(re, im)
        r, i = re.clone(), im.clone()
        ore, oim = fn(r, i, out=(r, i))
        assert ore is r and oim is i and eq(r, fre) and eq(i, fim), (dt, name)
    fre, fim = p.forward(re)
    r, i = re.clone(), torch.empty_like(re)
    p.forward(r, None, out=(r, i))
    assert eq(r, fre) and eq(i, fim), (dt, "forward(real)")
    z = torch.complex(re, im)
    fresh = p.forward_interleaved(z)
    zz = z.clone()
    assert p.forward_interleaved(zz, out=zz) is zz and eq(torch.view_as_real(zz), torch.view_as_real(fresh)), dt
    frames = torch.randn((batch, n), dtype=tdt, device="cuda:0", generator=g)
    keep = frames.clone()
    bins = n // 2 + 1
    view = frames.reshape(-1)[n:n + batch * bins].view(batch, bins)  # an output one row into the frames
    with pytest.raises(PdspError) as e:
        p.spectrum(frames, out=view)
    assert e.value.code == BAD and str(e.value) == TEXT_SPECTRUM.decode(), str(e.value)
    torch.cuda.synchronize()
    assert eq(frames, keep)
    with pytest.raises(PdspError) as e:  # re_out one row into re_in
        p.forward(re[:4], im[:4], out=(re[1:], torch.empty_like(im[:4])))
    assert e.value.code == BAD and str(e.value) == TEXT_PLANAR.decode(), str(e.value)

"""The stand-alone element-wise kernels of pdsp_elementwise_kernel.h (apply_window_kernel, polar_kernel, complex_op_kernel),
their launchers and their entry points, path by path against numpy f64 references computed from the same inputs
rounded to the dtype.

Paths.  complex_op_kernel has two instantiations per op: V = 4 (16-byte accesses) and V = 1.  _vec4() mirrors the
predicate of launch_complex_op and is asserted in every case, together with the launcher's own answer
(pdsp_dev_complex_op_vec4), so a change of the dispatch rule fails here and does not silently move a case to the other
kernel.  grid_for caps a grid at 2048 x 256 = CAP threads, so only a count above
CAP (V = 1) or 4 CAP (V = 4) sends a thread round the grid-stride loop a second time.

Inputs.  Magnitudes uniform in log2 over [2^-20, 2^20] with random signs, divisors included: every product, sum of
squares and quotient below is a normal number, so the bounds hold without exceptions, and no bound is helped by large
elements hiding small ones.

Bounds, per output component, u = 2^-24.  They are derived, not measured.
  add, sub, conj, scale   one correctly rounded operation or a sign flip: bitwise equal to the numpy float32 operation.
  mul, mulScalar          a real part is fl(fl(p1) - fl(p2)) with p1 = ar br, p2 = ai bi:
                          p1 (1 + d1) - p2 (1 + d2), all of it times (1 + d3), |d| <= u, so
                          |got - exact| <= u (|p1| + |p2|) + u (1 + u)(|p1| + |p2|) = (2u + u^2) S with S = |p1| + |p2|;
                          the imaginary part likewise with the cross terms.  The explicit fma of complex_op1 drops one
                          rounding and only does better.  divScalar is mulScalar by the reciprocal computed on the host
                          in double and rounded to f32, and its reference is computed that way.
  div                     num as above: |dnum| <= (2u + u^2) S.  den = br^2 + bi^2 has only positive terms, so
                          den^ = den (1 + e), |e| <= 2u + u^2.  The quotient is correctly rounded (hipcc's default for
                          f32 division): got = num^ / den^ (1 + d).  With |num| <= S that is
                          |got - exact| <= (S / den) (2u + 2u + u) to first order; the sixth u covers the
                          second-order terms (at most some 15 u^2).  Bound: 6u S / den.
  magnitude f32           within 1 ulp of hypot in f64, the ulp that of the reference rounded to f32 (the header's
                          contract, measured as test_magnitude_range_edges does).
  magnitude f64           2 ulp, phase f64 3 ulp (as test_gpu_batch_checks.py).
  phase f32               |wrap(got - arctan2_f64)| <= 4 * 2^-23, what test_gpu_hilbert.py allows the same atan2.
  apply_window            one correctly rounded product: bitwise equal to x * w in the dtype.
The f64 references themselves are exact products (48 bits) and one f64 rounding of their sum, 2^-53 S: 2^-29 of the
f32 bounds.

Each case prints the worst ratio of error to bound as an ELEMERR line."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CAP = 2048 * 256  # grid_for: at most this many threads
OPS = ["add", "sub", "mul", "div", "conj", "scale", "mulScalar"]
BINARY = ("add", "sub", "mul", "div")
SCALARS = {"scale": (1.7, 0.0), "mulScalar": (0.3, -1.9)}
N_SCALAR = 2 * CAP + 3           # V = 1: every thread twice, three of them a third time
N_VEC4 = 4 * (2 * CAP + 5)       # V = 4: the same in units of four
B_LEN = 4 * 1021                 # broadcast row on the V = 4 path
N_BCAST = B_LEN * 514            # the first multiple of B_LEN above 4 CAP
assert N_BCAST > 4 * CAP >= N_BCAST - B_LEN
NAN = float("nan")


def _vec4(op, a, b, out, count, b_len):
    """Mirror of the vec4 predicate of launch_complex_op (pdsp_dispatch.inc); a, b, out are pairs of addresses."""
    binary = op in BINARY
    return (all(p % 16 == 0 for p in (*a, *out)) and (not binary or all(p % 16 == 0 for p in b)) and count % 4 == 0
            and (not binary or b_len % 4 == 0))


def draw(rng, n, dtype=np.float32):
    return (np.exp2(rng.uniform(-20, 20, n)) * rng.choice([-1.0, 1.0], n)).astype(dtype)


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.cpu().numpy()


def shifted(t, off=1):
    """A copy of the 1-D tensor `t` that begins `off` elements into a fresh (256-byte aligned) allocation."""
    import torch
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=t.device)
    v = buf[off:]
    v.copy_(t)
    return v


def blank(n, dtype=None):
    """An output of `n` NaNs (or one shaped like the tensor `n`): an element the kernel skips cannot hold a stale
    right answer from an earlier allocation."""
    import torch
    if isinstance(n, torch.Tensor):
        return torch.full_like(n, NAN)
    return torch.full((n,), NAN, dtype=dtype or torch.float32, device="cuda")


def bits(t):
    import torch
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64)


@pytest.fixture(scope="module")
def lib():
    import pragma_dsp_amd
    return pragma_dsp_amd.lib


@pytest.fixture(scope="module")
def big():
    """The module's inputs, drawn once: four f32 planes of N_VEC4 values, host and device.  Never written to."""
    rng = np.random.default_rng(2024)
    h = {k: draw(rng, N_VEC4) for k in ("ar", "ai", "br", "bi")}
    d = {k: dev(v) for k, v in h.items()}
    for v in d.values():
        assert v.data_ptr() % 16 == 0
    return h, d


def cx(lib, op, a, b=None, out=None, count=None, b_len=None, vec4=None):
    """pdsp_complex_op_f32 on pairs of 1-D device tensors.  `vec4` is the path the case is meant for: asserted."""
    import torch
    from pragma_dsp_amd import _capi
    count = a[0].numel() if count is None else count
    if out is None:
        out = (blank(count), blank(count))
    if b_len is None:
        b_len = b[0].numel() if b is not None else 0
    pa = tuple(t.data_ptr() for t in a)
    pb = tuple(t.data_ptr() for t in b) if b is not None else (0, 0)
    po = tuple(t.data_ptr() for t in out)
    assert vec4 is not None and _vec4(op, pa, pb, po, count, b_len) is vec4, (op, count, b_len)
    s_re, s_im = SCALARS.get(op, (0.0, 0.0))
    vp = C.c_void_p
    chosen = C.c_int(-1)  # ... and the launcher's own rule says the same
    _capi.check(lib.pdsp_dev_complex_op_vec4(_capi.COMPLEX_OPS[op], count, vp(pa[0]), vp(pa[1]), vp(pb[0] or None),
                                             vp(pb[1] or None), b_len, vp(po[0]), vp(po[1]), C.byref(chosen)))
    assert chosen.value == int(vec4), (op, count, b_len)
    _capi.check(lib.pdsp_complex_op_f32(_capi.COMPLEX_OPS[op], count, vp(pa[0]), vp(pa[1]), vp(pb[0] or None),
                                        vp(pb[1] or None), b_len, s_re, s_im, vp(po[0]), vp(po[1]),
                                        vp(torch.cuda.current_stream().cuda_stream)))
    return out


def reference(op, ar, ai, br=None, bi=None, scalars=None):
    """(exact_re, exact_im, bound_re, bound_im) in f64, or for the bitwise ops (want_re, want_im, None, None) in f32.
    br / bi are full length (a broadcast row tiled by the caller)."""
    if op in ("scale", "mulScalar"):
        s = SCALARS[op] if scalars is None else scalars
        br, bi = np.float32(s[0]), np.float32(s[1])
    if op == "add":
        return ar + br, ai + bi, None, None
    if op == "sub":
        return ar - br, ai - bi, None, None
    if op == "conj":
        return ar.copy(), -ai, None, None
    if op == "scale":
        return ar * br, ai * br, None, None
    ar, ai, br, bi = (np.asarray(v, np.float64) for v in (ar, ai, br, bi))
    if op in ("mul", "mulScalar"):
        k = 2 * U + U * U
        return (ar * br - ai * bi, ar * bi + ai * br, k * (np.abs(ar * br) + np.abs(ai * bi)),
                k * (np.abs(ar * bi) + np.abs(ai * br)))
    assert op == "div"
    den = br * br + bi * bi
    return ((ar * br + ai * bi) / den, (ai * br - ar * bi) / den, 6 * U * (np.abs(ar * br) + np.abs(ai * bi)) / den,
            6 * U * (np.abs(ai * br) + np.abs(ar * bi)) / den)


def judge(op, case, got, ref):
    """Assert one result against reference(); print and return the worst ratio of error to bound (0 if bitwise)."""
    gr, gi = (host(t) for t in got)
    wr, wi, b_re, b_im = ref
    if b_re is None:
        assert np.array_equal(gr.view(np.int32), wr.view(np.int32)), (op, case, "re")
        assert np.array_equal(gi.view(np.int32), wi.view(np.int32)), (op, case, "im")
        print(f"ELEMERR {op} {case} bitwise")
        return 0.0
    assert np.isfinite(gr).all() and np.isfinite(gi).all(), (op, case)
    ratio = max(float((np.abs(gr - wr) / b_re).max()), float((np.abs(gi - wi) / b_im).max()))
    print(f"ELEMERR {op} {case} worst err/bound {ratio:.3f}")
    assert ratio <= 1.0, (op, case, ratio)
    return ratio


# ---- 1. the second trip round the grid-stride loops ---------------------------------------------------------------

@pytest.mark.parametrize("op", OPS)
def test_grid_stride_complex_op(lib, big, op):
    h, d = big
    binary = op in BINARY
    # V = 1: count % 4 == 3
    n = N_SCALAR
    got = cx(lib, op, (d["ar"][:n], d["ai"][:n]), (d["br"][:n], d["bi"][:n]) if binary else None, vec4=False)
    judge(op, "scalar", got, reference(op, h["ar"][:n], h["ai"][:n], h["br"][:n], h["bi"][:n]))
    # V = 4, b as long as a
    got = cx(lib, op, (d["ar"], d["ai"]), (d["br"], d["bi"]) if binary else None, vec4=True)
    judge(op, "vec4", got, reference(op, h["ar"], h["ai"], h["br"], h["bi"]))
    if not binary:
        return
    # V = 4 with a broadcast row: the index ((i * V) % b_len) / V on every trip
    n = N_BCAST
    got = cx(lib, op, (d["ar"][:n], d["ai"][:n]), (d["br"][:B_LEN], d["bi"][:B_LEN]), vec4=True)
    tile = [np.tile(h[k][:B_LEN], n // B_LEN) for k in ("br", "bi")]
    judge(op, "vec4-broadcast", got, reference(op, h["ar"][:n], h["ai"][:n], *tile))


def _t(dt):
    import torch
    return torch.float32 if dt == "f32" else torch.float64


def _np(dt):
    return np.float32 if dt == "f32" else np.float64


def window(lib, frames, win, out, batch, n):
    import torch
    from pragma_dsp_amd import _capi
    vp = C.c_void_p
    f = lib.pdsp_apply_window_f32 if frames.element_size() == 4 else lib.pdsp_apply_window_f64
    _capi.check(f(batch, n, vp(frames.data_ptr()), vp(win.data_ptr()), vp(out.data_ptr()),
                  vp(torch.cuda.current_stream().cuda_stream)))
    return out


def polar(lib, name, re, im, out, count=None):
    import torch
    from pragma_dsp_amd import _capi
    vp = C.c_void_p
    f = getattr(lib, f"pdsp_{name}_" + ("f32" if re.element_size() == 4 else "f64"))
    _capi.check(f(re.numel() if count is None else count, vp(re.data_ptr()), vp(im.data_ptr()), vp(out.data_ptr()),
                  vp(torch.cuda.current_stream().cuda_stream)))
    return out


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("n", [1021, 1])
def test_grid_stride_apply_window(lib, big, dt, n):
    import torch
    h, d = big
    batch = (2 * CAP) // n + 1 if n > 1 else N_SCALAR
    assert batch * n > 2 * CAP
    x = h["ar"][:batch * n].astype(_np(dt))
    w = h["br"][:n].astype(_np(dt))
    if dt == "f64":  # full-width mantissas, not f32 values in doubles
        x = x * (1 + h["ai"][:batch * n].astype(np.float64) * 2.0 ** -45)
        w = w * (1 + h["bi"][:n].astype(np.float64) * 2.0 ** -45)
    dx, dw = dev(x), dev(w)
    got = window(lib, dx, dw, blank(dx), batch, n)
    want = (x.reshape(batch, n) * w).reshape(-1)
    assert want.dtype == _np(dt)
    ib = np.int32 if dt == "f32" else np.int64
    assert np.array_equal(host(got).view(ib), want.view(ib))
    print(f"ELEMERR apply_window {dt} n={n} bitwise")
    # the Python caller, on the same rows
    from pragma_dsp_amd import batch as B
    assert torch.equal(B.apply_window(dx.view(batch, n), dw).view(-1), got)


def polar_inputs(big, dt, n):
    h, _ = big
    re, im = h["ar"][:n].astype(_np(dt)), h["ai"][:n].astype(_np(dt))
    if dt == "f64":
        re = re * (1 + h["br"][:n].astype(np.float64) * 2.0 ** -45)
        im = im * (1 + h["bi"][:n].astype(np.float64) * 2.0 ** -45)
    return re, im


def judge_polar(name, dt, case, got, re, im):
    """Assert magnitude / phase against the f64 reference at the bound of the module docstring; print the ratio."""
    got = got.astype(np.float64)
    re, im = re.astype(np.float64), im.astype(np.float64)
    if name == "magnitude":
        want = np.hypot(re, im)
        ulp = np.spacing(want.astype(_np(dt))).astype(np.float64)
        ratio = float((np.abs(got - want) / ((1 if dt == "f32" else 2) * ulp)).max())
    else:
        want = np.arctan2(im, re)
        if dt == "f32":
            dphi = np.angle(np.exp(1j * (got - want)))
            ratio = float((np.abs(dphi) / (4 * 2.0 ** -23)).max())
        else:
            ratio = float((np.abs(got - want) / (3 * np.spacing(np.abs(want)))).max())
    print(f"ELEMERR {name} {dt} {case} worst err/bound {ratio:.3f}")
    assert ratio <= 1.0, (name, dt, case, ratio)
    return ratio


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("name", ["magnitude", "phase"])
def test_grid_stride_polar(lib, big, name, dt):
    import torch
    re, im = polar_inputs(big, dt, N_SCALAR)
    dre, dim = dev(re), dev(im)
    got = polar(lib, name, dre, dim, blank(dre))
    judge_polar(name, dt, "grid-stride", host(got), re, im)
    from pragma_dsp_amd import batch as B
    assert torch.equal(getattr(B, name)(dre, dim), got)


# ---- 2. every condition of the vec4 predicate, one at a time ------------------------------------------------------

def test_each_vec4_condition_alone(lib, big):
    import torch
    h, d = big
    n = 4 * 1024
    a = (d["ar"][:n], d["ai"][:n])
    b = (d["br"][:n], d["bi"][:n])
    for op in ("mul", "scale"):
        binary = op in BINARY
        bb = b if binary else None
        base = cx(lib, op, a, bb, vec4=True)
        judge(op, "predicate-base", base, reference(op, h["ar"][:n], h["ai"][:n], h["br"][:n], h["bi"][:n]))
        # each pointer alone, one element off a 16-byte boundary
        for which in (("a", 0), ("a", 1), ("b", 0), ("b", 1), ("out", 0), ("out", 1)):
            if which[0] == "b" and not binary:
                continue
            aa, b2 = list(a), list(b)
            out = [blank(n), blank(n)]
            if which[0] == "a":
                aa[which[1]] = shifted(aa[which[1]])
            elif which[0] == "b":
                b2[which[1]] = shifted(b2[which[1]])
            else:
                out[which[1]] = blank(n + 1)[1:]
            got = cx(lib, op, tuple(aa), tuple(b2) if binary else None, out=tuple(out), vec4=False)
            assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), (op, which)
        # count % 4 != 0, every pointer aligned
        for r in (1, 2, 3):
            m = n + r
            got = cx(lib, op, (d["ar"][:m], d["ai"][:m]), (d["br"][:m], d["bi"][:m]) if binary else None, vec4=False)
            assert torch.equal(got[0][:n], base[0]) and torch.equal(got[1][:n], base[1]), (op, r)
            judge(op, f"count%4={r}", got, reference(op, h["ar"][:m], h["ai"][:m], h["br"][:m], h["bi"][:m]))
    # count % 4 == 0 but b_len % 4 != 0: the broadcast on the scalar path, against the same row tiled (vec4)
    n, b_len = 6 * 512, 6
    a = (d["ar"][:n], d["ai"][:n])
    row = (d["br"][:b_len], d["bi"][:b_len])
    tiled = tuple(t.repeat(n // b_len) for t in row)
    base = cx(lib, "mul", a, tiled, vec4=True)
    got = cx(lib, "mul", a, row, vec4=False)
    assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    judge("mul", "b_len=6", got, reference("mul", h["ar"][:n], h["ai"][:n], host(tiled[0]), host(tiled[1])))


# ---- 3. the two instantiations agree bit for bit -------------------------------------------------------------------

@pytest.mark.parametrize("op", OPS)
def test_paths_agree_bit_for_bit(lib, big, op):
    import torch
    _, d = big
    n = 4 * 1024
    a = (d["ar"][:n], d["ai"][:n])
    binary = op in BINARY
    for b_len in ((n, 4 * 256) if binary else (0,)):
        b = (d["br"][:b_len], d["bi"][:b_len]) if binary else None
        fast = cx(lib, op, a, b, vec4=True)
        sa = tuple(shifted(t) for t in a)
        sb = tuple(shifted(t) for t in b) if binary else None
        so = (blank(n + 1)[1:], blank(n + 1)[1:])
        slow = cx(lib, op, sa, sb, out=so, vec4=False)
        for k in (0, 1):
            assert torch.equal(bits(fast[k]), bits(slow[k])), (op, b_len, "re" if k == 0 else "im")


# ---- 4. broadcast ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", ["mul", "div"])
@pytest.mark.parametrize("b_len", [1, 4, 1021, 4096])
def test_broadcast_against_tile(lib, big, op, b_len):
    import torch
    h, d = big
    n = 12 if b_len <= 4 else 3 * b_len
    a = (d["ar"][:n], d["ai"][:n])
    off = 100  # the row is not the head of the planes a comes from
    row_h = [h[k][off:off + b_len] for k in ("br", "bi")]
    row = tuple(dev(v) for v in row_h)
    got = cx(lib, op, a, row, vec4=(b_len % 4 == 0))
    tile = [np.tile(v, n // b_len) for v in row_h]
    judge(op, f"b_len={b_len}", got, reference(op, h["ar"][:n], h["ai"][:n], *tile))
    full = cx(lib, op, a, tuple(dev(v) for v in tile), vec4=(n % 4 == 0))  # b_len == count: no index arithmetic
    assert torch.equal(bits(got[0]), bits(full[0])) and torch.equal(bits(got[1]), bits(full[1]))


@pytest.mark.parametrize("op", OPS)
def test_python_callers_against_the_oracle(lib, big, oracle_mod, op):
    """batch.py's callers at one shape (3 x 1024, a broadcast row for mul and div as well), at the bounds above, with
    the reference's own restatement (oracle.complex_op, in f64) in the loop."""
    from pragma_dsp_amd import batch as B
    h, d = big
    rows, n = 3, 1024
    cnt = rows * n
    ar, ai, br, bi = (h[k][:cnt].reshape(rows, n) for k in ("ar", "ai", "br", "bi"))
    da = (d["ar"][:cnt].view(rows, n), d["ai"][:cnt].view(rows, n))
    db = (d["br"][:cnt].view(rows, n), d["bi"][:cnt].view(rows, n))
    s = SCALARS.get(op, (0.0, 0.0))
    fn = {"add": B.complex_add, "sub": B.complex_sub, "mul": B.complex_mul, "div": B.complex_div}
    if op in BINARY:
        got = fn[op](da, db)
        want = oracle_mod.complex_op(op, ar, ai, br, bi)
    elif op == "conj":
        got, want = B.complex_conj(da), oracle_mod.complex_op("conj", ar, ai)
    elif op == "scale":
        got, want = B.complex_scale(da, s[0]), oracle_mod.complex_op("scale", ar, ai, s_re=float(np.float32(s[0])))
    else:
        got = B.complex_mul_scalar(da, *s)
        want = oracle_mod.complex_op("mulScalar", ar, ai, s_re=float(np.float32(s[0])), s_im=float(np.float32(s[1])))

    def against_oracle(op, case, got, want, ref):
        wr, wi, b_re, b_im = ref
        if b_re is None:  # exact in f32, and the oracle's f64 value rounds to it
            b_re, b_im = (np.abs(v).astype(np.float64) * U for v in (wr, wi))
        gr, gi = (host(t).astype(np.float64).reshape(-1) for t in got)
        r = max(float((np.abs(gr - want[0].reshape(-1)) / np.maximum(b_re, 1e-300)).max()),
                float((np.abs(gi - want[1].reshape(-1)) / np.maximum(b_im, 1e-300)).max()))
        print(f"ELEMERR {op} {case} worst err/bound {r:.3f}")
        assert r <= 1.0, (op, case, r)

    flat = [v.reshape(-1) for v in (ar, ai, br, bi)]
    ref = reference(op, *flat)
    judge(op, "python", tuple(t.reshape(-1) for t in got), ref)
    against_oracle(op, "oracle", got, want, ref)
    if op in ("mul", "div"):
        got = fn[op](da, (db[0][1], db[1][1]))  # row 1 of b over every row of a
        want = oracle_mod.complex_op(op, ar, ai, br[1], bi[1])
        ref = reference(op, flat[0], flat[1], np.tile(br[1], rows), np.tile(bi[1], rows))
        against_oracle(op, "oracle-broadcast", got, want, ref)
    if op == "mulScalar":  # divScalar: mulScalar by the host-computed reciprocal, rounded to f32
        re, im = 3.0, 4.0
        got = B.complex_div_scalar(da, re, im)
        den = re * re + im * im
        judge("divScalar", "python", tuple(t.reshape(-1) for t in got),
              reference("mulScalar", flat[0], flat[1], scalars=(re / den, -im / den)))
        want = oracle_mod.complex_op("div", ar, ai, [re], [im])
        # the oracle divides in f64; the rounded reciprocal is within u of 1 / (re + i im) per component, and both are
        # used twice over: 2u S more, S <= (|ar| + |ai|) max(|s_re|, |s_im|) (1 + u)
        gr, gi = (host(t).astype(np.float64) for t in got)
        S = (np.abs(ar) + np.abs(ai)).astype(np.float64) * max(abs(re), abs(im)) / den
        assert (np.abs(gr - want[0].reshape(rows, n)) <= (4 * U + 3 * U * U) * S).all()
        assert (np.abs(gi - want[1].reshape(rows, n)) <= (4 * U + 3 * U * U) * S).all()


# ---- 5. guard bands -------------------------------------------------------------------------------------------------

PAD = 8  # elements of NaN in front of an output: a multiple of 16 bytes, so offset 0 stays aligned


def banded(n, off, dtype=None):
    """(buffer, view): `n` elements that begin PAD + off elements into a NaN-filled buffer with PAD + 3 behind."""
    import torch
    buf = torch.full((PAD + off + n + PAD + 3,), NAN, dtype=dtype or torch.float32, device="cuda")
    return buf, buf[PAD + off:PAD + off + n]


def bands_intact(buf, before, n, off):
    import torch
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=buf.device)
    mask[PAD + off:PAD + off + n] = False
    return torch.equal(bits(buf)[mask], bits(before)[mask])


@pytest.mark.parametrize("op", OPS)
def test_guard_bands_complex_op(lib, big, op):
    import torch
    _, d = big
    binary = op in BINARY
    for n in (4 * 257, 4 * 257 + 3):
        a = (d["ar"][:n], d["ai"][:n])
        b = (d["br"][:n], d["bi"][:n]) if binary else None
        ref = cx(lib, op, a, b, vec4=(n % 4 == 0))
        for off in (0, 1):
            (bre, ore), (bim, oim) = banded(n, off), banded(n, off)
            before = bre.clone()
            got = cx(lib, op, a, b, out=(ore, oim), vec4=(n % 4 == 0 and off == 0))
            torch.cuda.synchronize()
            assert torch.equal(bits(got[0]), bits(ref[0])) and torch.equal(bits(got[1]), bits(ref[1])), (op, n, off)
            assert bands_intact(bre, before, n, off) and bands_intact(bim, before, n, off), (op, n, off)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_guard_bands_window_and_polar(lib, big, dt):
    import torch
    for n in (4 * 257, 4 * 257 + 3):
        re, im = (dev(v) for v in polar_inputs(big, dt, n))
        w = re[:257].clone()
        refs = {"window": window(lib, re[:4 * 257], w, blank(4 * 257, _t(dt)), 4, 257),
                "magnitude": polar(lib, "magnitude", re, im, blank(re)),
                "phase": polar(lib, "phase", re, im, blank(re))}
        for off in (0, 1):
            for name, ref in refs.items():
                m = ref.numel()
                buf, out = banded(m, off, _t(dt))
                before = buf.clone()
                if name == "window":
                    window(lib, re[:m], w, out, 4, 257)
                else:
                    polar(lib, name, re, im, out)
                torch.cuda.synchronize()
                assert torch.equal(bits(out), bits(ref)), (name, n, off)
                assert bands_intact(buf, before, m, off), (name, n, off)


# ---- 6. allowed aliasing: bitwise equal to out of place ------------------------------------------------------------

@pytest.mark.parametrize("path", ["vec4", "scalar"])
def test_allowed_aliasing_complex_op(lib, big, path):
    import torch
    _, d = big
    n = 4 * 1024 if path == "vec4" else 4 * 1024 + 3
    v = path == "vec4"

    def fresh():
        return (d["ar"][:n].clone(), d["ai"][:n].clone()), (d["br"][:n].clone(), d["bi"][:n].clone())

    def same(x, y):
        return torch.equal(bits(x[0]), bits(y[0])) and torch.equal(bits(x[1]), bits(y[1]))

    for op in OPS:
        binary = op in BINARY
        a, b = fresh()
        ref = cx(lib, op, a, b if binary else None, vec4=v)
        got = cx(lib, op, a, b if binary else None, out=a, vec4=v)  # out = a
        assert got[0].data_ptr() == a[0].data_ptr() and same(a, ref), (op, "out = a")
        a, b = fresh()
        cx(lib, op, a, b if binary else None, out=(a[1], a[0]), vec4=v)  # out_re = a_im, out_im = a_re
        assert same((a[1], a[0]), ref), (op, "out planes on the other planes of a")
        if binary:
            a, b = fresh()
            cx(lib, op, a, b, out=b, vec4=v)  # out = b, b_len == count
            assert same(b, ref), (op, "out = b")
            a, b = fresh()
            sq = cx(lib, op, a, a, vec4=v)
            cx(lib, op, a, a, out=a, vec4=v)  # a = b = out
            assert same(a, sq), (op, "a = b = out")
    # the square through the chain
    from pragma_dsp_amd.fluent import DeviceChain
    a, _ = fresh()
    sq = cx(lib, "mul", a, a, vec4=v)
    c = DeviceChain(a[0], a[1])
    assert c.mul(c) is c and same(c.unwrap(), sq)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_allowed_aliasing_window_and_polar(lib, big, dt):
    import torch
    from pragma_dsp_amd import batch as B
    rows, n = 5, 1021
    re, im = (dev(v).view(rows, n) for v in polar_inputs(big, dt, rows * n))
    w = im[2].clone()
    ref = B.apply_window(re, w)
    x = re.clone()
    assert B.apply_window(x, w, out=x) is x and torch.equal(bits(x), bits(ref))
    ref = B.magnitude(re, im)
    x = re.clone()
    assert B.magnitude(x, im, out=x) is x and torch.equal(bits(x), bits(ref))
    y = im.clone()
    assert B.magnitude(re, y, out=y) is y and torch.equal(bits(y), bits(ref))
    ref = B.phase(re, im)
    y = im.clone()
    assert B.phase(re, y, out=y) is y and torch.equal(bits(y), bits(ref))
    x = re.clone()
    assert B.phase(x, im, out=x) is x and torch.equal(bits(x), bits(ref))
    x = re.clone()  # re == im == out
    assert torch.equal(bits(B.magnitude(x, x, out=x)), bits(B.magnitude(re, re)))


# ---- 7. refused aliasing --------------------------------------------------------------------------------------------

def refused(fn, *buffers):
    """fn() must raise "output overlaps input" and leave every one of `buffers` as it was."""
    import torch
    from pragma_dsp_amd import PdspError, _capi
    before = [t.clone() for t in buffers]
    with pytest.raises(PdspError) as e:
        fn()
    assert e.value.code == _capi.ERR_BAD_ARG and "output overlaps input" in str(e.value)
    torch.cuda.synchronize()
    for t, was in zip(buffers, before):
        assert torch.equal(bits(t), bits(was))


def test_refused_aliasing(lib, big):
    import torch
    from pragma_dsp_amd import batch as B
    from pragma_dsp_amd.fluent import DeviceChain
    _, d = big
    rows, n = 4, 256
    cnt = rows * n
    buf = torch.empty(6 * cnt + 8, device="cuda")
    buf.copy_(d["ar"][:buf.numel()])
    a = (buf[:cnt], buf[cnt:2 * cnt])
    b = (d["br"][:cnt], d["bi"][:cnt])
    free = buf[3 * cnt:4 * cnt]
    for op in ("mul", "conj"):
        bb = b if op in BINARY else None
        # out = a shifted by one element, in either plane and either direction
        refused(lambda: cx(lib, op, a, bb, out=(buf[1:cnt + 1], free), vec4=False), buf)
        refused(lambda: cx(lib, op, a, bb, out=(free, buf[cnt + 1:2 * cnt + 1]), vec4=False), buf)
        refused(lambda: cx(lib, op, (buf[1:cnt + 1], a[1]), bb, out=(buf[:cnt], free), vec4=False), buf)
        # out_re meeting out_im: the same plane, and one element of overlap
        refused(lambda: cx(lib, op, a, bb, out=(free, free), vec4=True), buf)
        refused(lambda: cx(lib, op, a, bb, out=(free, buf[4 * cnt - 1:5 * cnt - 1]), vec4=False), buf)
        # one element past the end is accepted: out_re directly behind a_im, out_im directly behind out_re
        want = cx(lib, op, a, bb, vec4=True)
        got = cx(lib, op, a, bb, out=(buf[2 * cnt:3 * cnt], buf[3 * cnt:4 * cnt]), vec4=True)
        assert torch.equal(bits(got[0]), bits(want[0])) and torch.equal(bits(got[1]), bits(want[1]))
    # b of full length shifted against out
    refused(lambda: cx(lib, "add", a, (buf[2 * cnt:3 * cnt], b[1]),
                       out=(buf[2 * cnt + 4:3 * cnt + 4], buf[5 * cnt:6 * cnt]), vec4=True), buf)
    # a broadcast b that is row 0 of out: through the C entry, batch.py and the chain
    X = (buf[:cnt].view(rows, n), buf[cnt:2 * cnt].view(rows, n))
    refused(lambda: cx(lib, "div", a, (a[0][:n], a[1][:n]), out=a, vec4=True), buf)
    refused(lambda: B.complex_div(X, (X[0][0], X[1][0]), out=X), buf)
    refused(lambda: B.complex_mul(X, (X[0][2], d["bi"][:n]), out=X), buf)  # one plane of b, a later row
    c = DeviceChain(*X)
    refused(lambda: c.div((c.re[0], c.im[0])), buf)
    refused(lambda: c.mul((c.re[0], c.im[0])), buf)
    # ... while a copy of the row is the way to do it
    row = (c.re[0].clone(), c.im[0].clone())
    want = B.complex_div((X[0].clone(), X[1].clone()), row)
    c.div(row)
    assert torch.equal(bits(c.re), bits(want[0])) and torch.equal(bits(c.im), bits(want[1]))
    # a broadcast row that ends where out begins is accepted
    got = B.complex_mul((X[0][1:], X[1][1:]), (X[0][0], X[1][0]), out=(X[0][1:], X[1][1:]))
    assert got[0].data_ptr() == X[0][1].data_ptr()
    for dt in ("f32", "f64"):
        t = torch.empty(3 * cnt + 8, dtype=_t(dt), device="cuda")
        t.copy_(d["ai"][:t.numel()])
        x = t[:cnt].view(rows, n)
        w = d["br"][:n].to(_t(dt))
        # apply_window: out one element or one row further; the window inside out
        refused(lambda: B.apply_window(x, w, out=t[1:cnt + 1].view(rows, n)), t)
        refused(lambda: B.apply_window(x, w, out=t[n:cnt + n].view(rows, n)), t)
        refused(lambda: B.apply_window(x, x[1], out=x), t)
        refused(lambda: B.apply_window(t[cnt:2 * cnt].view(rows, n), x[rows - 1], out=x), t)
        want = B.apply_window(x, w)
        assert torch.equal(bits(B.apply_window(x, w, out=t[cnt:2 * cnt].view(rows, n))), bits(want))  # adjacent
        # magnitude / phase: out one element from re or from im
        im = t[2 * cnt:3 * cnt].view(rows, n)
        for fn in (B.magnitude, B.phase):
            refused(lambda: fn(x, im, out=t[1:cnt + 1].view(rows, n)), t)
            refused(lambda: fn(x, im, out=t[2 * cnt - 1:3 * cnt - 1].view(rows, n)), t)
            refused(lambda: fn(x, im, out=t[2 * cnt + 1:3 * cnt + 1].view(rows, n)), t)
            want = fn(x, im)
            assert torch.equal(bits(fn(x, im, out=t[cnt:2 * cnt].view(rows, n))), bits(want))  # between the two


# ---- 8. special values ----------------------------------------------------------------------------------------------

def test_division_by_zero_stays_in_its_element(lib, big):
    import torch
    h, d = big
    n = 4 * 64
    ar, ai, br, bi = (h[k][:n].copy() for k in ("ar", "ai", "br", "bi"))
    clean = cx(lib, "div", (dev(ar), dev(ai)), (dev(br), dev(bi)), vec4=True)
    t = np.float32(2.0 ** -80)  # its square underflows to zero: a zero denominator under a non-zero numerator
    z = np.float32(0.0)
    zeros = [(z, z), (-z, z), (z, -z), (-z, -z), (t, z), (-t, z), (z, t), (z, -t), (t, -t)]
    where = [5 + 9 * k for k in range(len(zeros))]  # every lane of a vector of four, with clean neighbours
    for i, (zr, zi) in zip(where, zeros):
        br[i], bi[i] = zr, zi
    ar[where[0]], ai[where[0]] = 1.5, -2.5
    for path in ("vec4", "scalar"):
        m = n if path == "vec4" else n - 1
        got = cx(lib, "div", (dev(ar[:m]), dev(ai[:m])), (dev(br[:m]), dev(bi[:m])), vec4=(path == "vec4"))
        with np.errstate(all="ignore"):
            den = br * br + bi * bi
            want = ((ar * br + ai * bi) / den)[:m], ((ai * br - ar * bi) / den)[:m]
        assert want[0].dtype == np.float32
        for g, w, c in zip(got, want, clean):
            g = host(g)
            assert not np.isfinite(w[where]).any()
            assert np.array_equal(np.isfinite(g), np.isfinite(w)), path
            assert np.array_equal(np.isnan(g), np.isnan(w)), path
            inf = np.isinf(w)
            assert inf.any() and np.array_equal(np.sign(g[inf]), np.sign(w[inf])), path
            keep = np.ones(m, bool)
            keep[where] = False
            assert np.array_equal(g[keep].view(np.int32), host(c)[:m][keep].view(np.int32)), path


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_phase_and_magnitude_special_values(lib, dt):
    import torch
    inf = float("inf")
    vals = [0.0, -0.0, 1.0, -1.0, inf, -inf]
    re = np.array([x for x in vals for _ in vals], _np(dt))
    im = np.array([y for _ in vals for y in vals], _np(dt))
    dre, dim = dev(re), dev(im)
    got = host(polar(lib, "phase", dre, dim, blank(dre))).astype(np.float64)
    want = np.arctan2(im.astype(np.float64), re.astype(np.float64))
    assert np.array_equal(np.signbit(got), np.signbit(want)), (re[np.signbit(got) != np.signbit(want)],
                                                               im[np.signbit(got) != np.signbit(want)])
    tol = 4 * 2.0 ** -23 if dt == "f32" else 3 * np.spacing(np.abs(want))
    assert (np.abs(got - want) <= tol).all()
    # spelled out, (im, re) -> sign and size: atan2(+-0, +0) = +-0, atan2(+-0, -0) = +-pi, atan2(+-0, -1) = +-pi
    table = [(0.0, 0.0, False, 0.0), (-0.0, 0.0, True, 0.0), (0.0, -0.0, False, np.pi), (-0.0, -0.0, True, np.pi),
             (0.0, -1.0, False, np.pi), (-0.0, -1.0, True, np.pi)]
    ti, tr = (dev(np.array([row[k] for row in table], _np(dt))) for k in (0, 1))
    got = host(polar(lib, "phase", tr, ti, blank(tr))).astype(np.float64)
    for g, (y, x, neg, size) in zip(got, table):
        assert bool(np.signbit(g)) == neg and abs(abs(g) - size) <= (4 * 2.0 ** -23 if size else 0.0), (y, x, g)
    # magnitude: the stated formula of each dtype decides what a NaN beside an infinity gives
    re = np.array([inf, NAN, NAN, 1.0, -inf, 3.0], _np(dt))
    im = np.array([NAN, 1.0, inf, NAN, 2.0, 4.0], _np(dt))
    got = host(polar(lib, "magnitude", dev(re), dev(im), blank(6, _t(dt))))
    with np.errstate(all="ignore"):
        want = np.sqrt(re * re + im * im) if dt == "f32" else np.hypot(re, im)
    assert np.isnan(want[:4]).sum() == (4 if dt == "f32" else 2)  # hypot lets an infinity win over a NaN
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))
    assert abs(got[5] - 5.0) <= 2 * np.spacing(_np(dt)(5.0))


def test_a_nan_changes_no_other_element(lib, big):
    import torch
    _, d = big
    n = 4 * 64
    for path in ("vec4", "scalar"):
        m = n if path == "vec4" else n - 1
        v = path == "vec4"
        a = (d["ar"][:m].clone(), d["ai"][:m].clone())
        b = (d["br"][:m].clone(), d["bi"][:m].clone())
        clean = {op: cx(lib, op, a, b if op in BINARY else None, vec4=v) for op in OPS}
        a[0][6] = NAN
        b[1][9] = NAN
        for op in OPS:
            got = cx(lib, op, a, b if op in BINARY else None, vec4=v)
            hit = [6, 9] if op in BINARY else [6]
            keep = torch.ones(m, dtype=torch.bool, device="cuda")
            keep[hit] = False
            for k in (0, 1):
                assert torch.equal(bits(got[k])[keep], bits(clean[op][k])[keep]), (op, path)
            assert bool(torch.isnan(got[0][6])), (op, path)
        # conj keeps a NaN a NaN and flips the sign of a zero
        a[1][3], a[1][4], a[1][5] = 0.0, -0.0, NAN
        got = cx(lib, "conj", a, vec4=v)
        assert bool(torch.signbit(got[1][3])) and not bool(torch.signbit(got[1][4])) and bool(torch.isnan(got[1][5]))
        assert bool(torch.isnan(got[0][6])) and torch.equal(bits(got[0])[:6], bits(a[0])[:6])
    for dt in ("f32", "f64"):
        re, im = (dev(x) for x in polar_inputs(big, dt, 257))
        w = im[:257].clone()
        bad = re.clone()
        bad[100] = NAN
        keep = torch.ones(257, dtype=torch.bool, device="cuda")
        keep[100] = False
        for name in ("magnitude", "phase"):
            clean = polar(lib, name, re, im, blank(re))
            got = polar(lib, name, bad, im, blank(re))
            assert torch.equal(bits(got)[keep], bits(clean)[keep]) and bool(torch.isnan(got[100])), (name, dt)
        clean = window(lib, re, w, blank(re), 1, 257)
        got = window(lib, bad, w, blank(re), 1, 257)
        assert torch.equal(bits(got)[keep], bits(clean)[keep]) and bool(torch.isnan(got[100])), dt


# ---- 9. counts 0 and 1 ---------------------------------------------------------------------------------------------

def test_counts_zero_and_one(lib, big):
    import torch
    h, d = big
    for op in OPS:
        binary = op in BINARY
        for count in (0, 1):
            (bre, ore), (bim, oim) = banded(count, 0), banded(count, 0)
            before = bre.clone()
            a = (d["ar"][:4], d["ai"][:4])
            b = (d["br"][:4], d["bi"][:4]) if binary else None
            cx(lib, op, a, b, out=(ore, oim), count=count, b_len=count if binary else 0,
               vec4=(count == 0))  # the predicate is met at count 0, where nothing is launched
            torch.cuda.synchronize()
            assert bands_intact(bre, before, count, 0) and bands_intact(bim, before, count, 0), (op, count)
            if count:
                judge(op, "count=1", (ore, oim), reference(op, *(h[k][:1] for k in ("ar", "ai", "br", "bi"))))
    for dt in ("f32", "f64"):
        re, im = (dev(v) for v in polar_inputs(big, dt, 8))
        for batch, n in ((0, 4), (4, 0), (0, 0), (1, 1)):
            buf, out = banded(batch * n, 0, _t(dt))
            before = buf.clone()
            window(lib, re, im, out, batch, n)
            torch.cuda.synchronize()
            assert bands_intact(buf, before, batch * n, 0), (dt, batch, n)
            if batch * n:
                assert torch.equal(out, re[:1] * im[:1])
        for name in ("magnitude", "phase"):
            for count in (0, 1):
                buf, out = banded(count, 0, _t(dt))
                before = buf.clone()
                polar(lib, name, re, im, out, count=count)
                torch.cuda.synchronize()
                assert bands_intact(buf, before, count, 0), (dt, name, count)
                assert not bool(torch.isnan(out).any())

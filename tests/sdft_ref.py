"""References for the sliding DFT (include/pdsp_hip.h, "sliding DFT"), written from its definition; no GPU, nothing of
the library.

    direct()   long double direct sums  Y[j][m] = sum_n w[n] x[m h + n] exp(-2 pi i b_j n / N)  with the exact phase
               rule and the window's cosine sum evaluated in long double -- of all frames, or of the frames asked for
    emulate()  the kernel's documented summation order (pdsp_sdft_kernel.h) in numpy, in f32 or f64, or with plain
               sequential scans of a chunk (order="sequential") as the yardstick the device's bound must stay below;
               with exact=True every fma is rounded once (fma32 / fma64): the device's bits, frame for frame
    sliding()  every frame of a rectangular bin from ONE long double prefix sum over the row: the full-coverage check
               (its own error is 2^-64 sqrt(T)-ish, three orders below f64's)

and the shapes the CPU and GPU tests share (SIZES, lengths, hops, bins_of, windows_of; PATH_SIZES and the path_*
functions of the path-by-path tests), their inputs and the error metric.  Reference values are cached per
case: the CPU test and the GPU tests of one session compute each once.
"""
import functools

import numpy as np

LD = np.longdouble
PI = 4 * np.arctan(LD(1))
WINDOWS = {"rect": (1.0,), "hann": (0.5, 0.5), "hamming": (0.54, 0.46), "blackman": (0.42, 0.5, 0.08)}
U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
DT = {"f32": np.float32, "f64": np.float64}
WG = 256


def segment(n, dtype):
    """E, the positions per thread (pdsp_internal.h, sdft_segment)."""
    return 8 if dtype == "f32" and n > 1024 else 4


def turns(i, b, mod):
    """((b i) mod `mod`) as long double, exactly: p = b i and its error term e (Dekker's split stands in for the fma),
    fmod of p, e added after the reduction."""
    i = np.asarray(i, dtype=np.float64)
    p = i * b
    c = 134217729.0 * b  # 2^27 + 1
    hi = c - (c - b)
    lo = b - hi
    e = (i * hi - p) + i * lo
    return np.fmod(p, mod).astype(LD) + e.astype(LD)


def phase_turns(n, b, c, i):
    """t1 +- t2 of component (b, c) at positions i: ((b i) mod N) / N +- ((|c| i) mod (N - 1)) / (N - 1)."""
    r = turns(i, float(b), float(n))
    t = np.where(r < 0, r + LD(n), r) / LD(n)  # fmod keeps a negative bin's sign: into [0, N)
    if c:
        t2 = ((abs(c) * np.asarray(i, dtype=np.int64)) % (n - 1)).astype(LD) / LD(n - 1)
        t = t - t2 if c < 0 else t + t2
    return t


def table(n, b, c=0):
    """exp(-2 pi i (t1 +- t2)) at i = 0 ... N in long double: (cos, sin)."""
    a = LD(-2) * PI * phase_turns(n, b, c, np.arange(n + 1))
    return np.cos(a), np.sin(a)


def window(name, n):
    """The library's window from its cosine sum, in long double (createWindow: N - 1 in the denominator)."""
    a = WINDOWS[name]
    f = 2 * PI * np.arange(n, dtype=LD) / LD(n - 1) if n > 1 else np.zeros(n, dtype=LD)
    w = np.full(n, LD(a[0]))
    for c in range(1, len(a)):
        w = w + (-1) ** c * LD(a[c]) * np.cos(c * f)
    return w


def components(name):
    """[(c, weight)] in table order: 0, +1, -1, +2, -2 with a_0, then (-1)^c a_c / 2."""
    a = WINDOWS[name]
    out = [(0, a[0])]
    for c in range(1, len(a)):
        out += [(c, (-1) ** c * a[c] / 2), (-c, (-1) ** c * a[c] / 2)]
    return out


def frames_of(n, hop, t):
    return 1 + (t - n) // hop if t >= n else 0


def direct(x, n, bins, hop=1, win="rect", frames=None):
    """complex long double [rows, K, len(frames)] as (re, im): the definition, frame by frame."""
    x = np.atleast_2d(np.asarray(x)).astype(LD)
    f = frames_of(n, hop, x.shape[1])
    frames = np.arange(f) if frames is None else np.asarray(frames)
    w = window(win, n)
    cs = [table(n, b) for b in bins]
    co = np.stack([c[0][:n] for c in cs], axis=1)  # [n, K]
    si = np.stack([c[1][:n] for c in cs], axis=1)
    re = np.empty((x.shape[0], len(bins), len(frames)), dtype=LD)
    im = np.empty_like(re)
    for k, m in enumerate(frames):
        seg = x[:, m * hop:m * hop + n] * w
        re[:, :, k] = seg @ co
        im[:, :, k] = seg @ si
    return re, im


def sliding(x, n, b, hop=1):
    """Every frame of the rectangular bin b from one long double prefix sum: Y[s] = e^(2 pi i b s / N) (P[s+N] - P[s]),
    P the prefix sums of x[t] e^(-2 pi i b t / N) with the phase of the exact rule.  (re, im) [rows, F]."""
    x = np.atleast_2d(np.asarray(x)).astype(LD)
    t = x.shape[1]
    a = LD(-2) * PI * phase_turns(n, b, 0, np.arange(t + 1))
    c, s = np.cos(a), np.sin(a)
    pr = np.concatenate([np.zeros((x.shape[0], 1), LD), np.cumsum(x * c[:t], axis=1)], axis=1)
    pi = np.concatenate([np.zeros((x.shape[0], 1), LD), np.cumsum(x * s[:t], axis=1)], axis=1)
    st = np.arange(frames_of(n, hop, t)) * hop
    dr, di = pr[:, st + n] - pr[:, st], pi[:, st + n] - pi[:, st]
    return dr * c[st] + di * s[st], di * c[st] - dr * s[st]  # times conj(e^(-i a))


# ---- the kernel's order in numpy ------------------------------------------------------------------------------------

def _two_sum(a, b):
    """(s, e) with s = fl(a + b) and s + e = a + b exactly (Knuth; f64, no overflow)."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _to_odd(s, e):
    """fl(a + b) rounded to odd, from TwoSum's (s, e): where the sum is inexact and s's last bit is even, the
    neighbour of s on e's side (it is odd, and the exact sum lies between the two)."""
    fix = (e != 0) & ((s.view(np.int64) & 1) == 0)
    return np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)


def _split(a):
    """Veltkamp: a = hi + lo, each of at most 26 significant bits."""
    c = 134217729.0 * a  # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def fma32(a, b, c):
    """fmaf(a, b, c) of f32 arrays, correctly rounded: the product is exact in f64 (48 bits), the sum is rounded to
    odd in f64 (53 >= 2 x 24 + 2 bits: the second rounding then sees what one rounding of the exact value sees)."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    a, b, c = np.broadcast_arrays(a, b, c)
    return _to_odd(*_two_sum(a * b, c)).astype(np.float32)


def fma64(a, b, c):
    """fma(a, b, c) of f64 arrays, correctly rounded (Boldo and Melquiond, "Emulation of a FMA and correctly rounded
    sums: proved algorithms using rounding to odd", 2008): a b = uh + ul exactly (Dekker's product on Veltkamp's
    split), c + uh = th + tl exactly, v = tl + ul rounded to odd, the result fl(th + v).  No overflow and no underflow
    in the domain: signals of O(1), tables whose nonzero entries are normal."""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (a, b, c)))
    uh = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    ul = al * bl - (((uh - ah * bh) - al * bh) - ah * bl)
    th, tl = _two_sum(c, uh)
    return th + _to_odd(*_two_sum(tl, ul))


class _Arith:
    """Arithmetic of one precision with the kernel's fused operations.  f32: products are exact in f64, so
    fma(a, b, c) = f32(f64(a) f64(b) + f64(c)) (a double rounding, one case in 2^29).  f64: numpy has no fma; a product
    and a sum stand in (two roundings where the device has one: the emulation's error is an upper estimate).
    exact: fma32 / fma64 above, one rounding as on the device -- the form the device is held to bit for bit."""

    def __init__(self, dtype, exact=False):
        self.t = DT[dtype]
        self.f32 = dtype == "f32"
        self.exact = exact

    def fma(self, a, b, c):
        if self.exact:
            return fma32(a, b, c) if self.f32 else fma64(a, b, c)
        if self.f32:
            return (a.astype(np.float64) * np.asarray(b, np.float64) + c.astype(np.float64)).astype(np.float32)
        return a * b + c

    def cmul(self, ar, ai, br, bi):
        return self.fma(-ai, bi, ar * br), self.fma(ai, br, ar * bi)


def _scan(v, axis_len, reverse):
    """Hillis-Steele over the last axis (64 lanes), ascending or mirrored, then the one-lane shift: (exclusive, total)."""
    v = v.copy()
    d = 1
    while d < axis_len:
        if reverse:
            v[..., :-d] = v[..., :-d] + v[..., d:]
        else:
            v[..., d:] = v[..., d:] + v[..., :-d]
        d *= 2
    ex = np.zeros_like(v)
    if reverse:
        ex[..., :-1] = v[..., 1:]
        return ex, v[..., 0]
    ex[..., 1:] = v[..., :-1]
    return ex, v[..., -1]


def _seq(tot, reverse):
    """0 + t_0 + ... + t_{k-1} for every k along the last axis (mirrored: 0 + t_last + ... + t_{k+1})."""
    out = np.zeros_like(tot)
    k = tot.shape[-1]
    if reverse:
        for j in range(k - 2, -1, -1):
            out[..., j] = out[..., j + 1] + tot[..., j + 1]
    else:
        for j in range(1, k):
            out[..., j] = out[..., j - 1] + tot[..., j - 1]
    return out


def _chunk_scans(ar, xs, tr, ti, e_seg, order):
    """xs [rows, chunks, npad] (zero beyond N), tr / ti [npad]: (Pex re, im, S re, im, each [rows, chunks, npad])."""
    t = ar.t
    if order == "sequential":
        zr, zi = xs * tr, xs * ti
        out = []
        for z in (zr, zi):
            inc = np.cumsum(z, axis=-1, dtype=t)
            out.append(np.concatenate([np.zeros_like(inc[..., :1]), inc[..., :-1]], axis=-1))
        for z in (zr, zi):
            out.append(np.cumsum(z[..., ::-1], axis=-1, dtype=t)[..., ::-1])
        return out
    rows, chunks, npad = xs.shape
    rounds = npad // (WG * e_seg)
    shape = (rows, chunks, rounds, WG // 64, 64, e_seg)
    x5 = xs.reshape(shape)
    t5r, t5i = tr.reshape(shape[2:]), ti.reshape(shape[2:])
    res = []
    totals = None
    for reverse in (False, True):
        part = []
        for tp in (t5r, t5i):
            loc = np.zeros(shape, dtype=t)  # lp_e (before e) or rs_e (down to e)
            run = np.zeros(shape[:-1], dtype=t)
            order_e = range(e_seg - 1, -1, -1) if reverse else range(e_seg)
            for e in order_e:
                if not reverse:
                    loc[..., e] = run
                run = ar.fma(x5[..., e], tp[..., e], run)
                if reverse:
                    loc[..., e] = run
            ex, wtot = _scan(run, 64, reverse)                 # [rows, chunks, rounds, waves, 64], [.., waves]
            wsum = _seq(wtot, reverse)                          # WP_w / WS_w
            base = wsum[..., None] + ex
            if rounds > 1:
                if not reverse:
                    rt = _seq(wtot, False)[..., -1] + wtot[..., -1]  # R = 0 + W_0 + W_1 + W_2 + W_3
                    totals = [rt] if totals is None else totals + [rt]
                    rsum = _seq(rt, False)
                else:
                    rsum = _seq(totals[len(part)], True)           # the R of the prefix scan of that chunk
                base = rsum[..., None, None] + base
            part.append((base[..., None] + loc).reshape(rows, chunks, npad))
        res += part
    return res


def emulate(x, n, bins, hop=1, win="rect", dtype="f32", order="device", exact=False):
    """complex [rows, K, F] in the precision's complex type: the kernel's arithmetic on the tables rounded once from
    long double.  exact: every fma with one rounding (fma32 / fma64), the device's bits."""
    ar = _Arith(dtype, exact)
    t = ar.t
    x = np.atleast_2d(np.asarray(x)).astype(t)
    rows, samples = x.shape
    f = frames_of(n, hop, samples)
    e_seg = segment(n, dtype)
    blk = WG * e_seg
    npad = -(-n // blk) * blk
    chunks = (samples - n) // n + 2  # the chunks with a start, and the one after
    xs = np.zeros((rows, chunks, npad), dtype=t)
    flat = np.zeros((rows, chunks * n), dtype=t)
    flat[:, :min(samples, chunks * n)] = x[:, :chunks * n]
    xs[:, :, :n] = flat.reshape(rows, chunks, n)
    st = np.arange(f) * hop
    cc, ii = st // n, st % n
    out = np.empty((rows, len(bins), f), dtype=np.complex64 if dtype == "f32" else np.complex128)
    for j, b in enumerate(bins):
        acc_r = acc_i = None
        for k, (c, wgt) in enumerate(components(win)):
            co, si = table(n, b, c)
            tr, ti = np.full(npad, co[n], dtype=t), np.full(npad, si[n], dtype=t)
            tr[:n], ti[:n] = co[:n].astype(t), si[:n].astype(t)
            tnr, tni = t(co[n]), t(si[n])
            pr, pi, sr, si_ = _chunk_scans(ar, xs, tr, ti, e_seg, order)
            # frame (c, i): v = S_c[i] + tab[N] Pex_{c+1}[i];  y = conj(tab[i]) v
            pr, pi, sr, si_ = pr[:, cc + 1, ii], pi[:, cc + 1, ii], sr[:, cc, ii], si_[:, cc, ii]
            mr, mi = ar.cmul(np.full_like(pr, tnr), np.full_like(pr, tni), pr, pi)
            vr, vi = sr + mr, si_ + mi
            yr, yi = ar.cmul(np.broadcast_to(tr[ii], vr.shape), np.broadcast_to(-ti[ii], vr.shape), vr, vi)
            w = t(wgt)
            if k == 0:
                acc_r, acc_i = w * yr, w * yi
            else:
                acc_r, acc_i = ar.fma(yr, w, acc_r), ar.fma(yi, w, acc_i)
        out.real[:, j, :], out.imag[:, j, :] = acc_r, acc_i  # (part by part: a sum with 1j * im loses a zero's sign)
    return out


# ---- the shapes, inputs and metric the tests share ------------------------------------------------------------------

SIZES = (2, 3, 63, 64, 65, 100, 1000, 4096, 16384)
WINDOWED = (64, 100, 4096)
ROWS = 3


def lengths(n):
    return (n, n + 1, 2 * n - 1, 2 * n, 2 * n + 1, 3 * n + 7)


def hops(n):
    return tuple(h for h in dict.fromkeys((1, 7, n - 1, n, n + 1, 2 * n + 5)) if h >= 1)


def bins_of(n):
    return (0.0, 1.0, n / 2, n - 1.0, 12.5, -3.0, n + 2.0)


def windows_of(n):
    return tuple(WINDOWS) if n in WINDOWED else ("rect",)


def signal(n, t, seed=0):
    """Seeded Gaussian rows [ROWS, t], exactly representable in f32 so that both precisions share one reference."""
    rng = np.random.default_rng([n, t, seed])
    return rng.standard_normal((ROWS, t)).astype(np.float32).astype(np.float64)


def pick_frames(n, hop, t, limit=32):
    """All frames where they are few; else the first and last, those whose starts straddle the chunk and round
    boundaries, and a seeded sample."""
    f = frames_of(n, hop, t)
    if f <= limit:
        return np.arange(f)
    m = {0, 1, f - 2, f - 1}
    for edge in list(range(0, t, n)) + [c * n + r for c in range(t // n + 1) for r in range(1024, n, 1024)]:
        for s in (edge - 1, edge, edge + 1):
            if s >= 0:
                m.update((s // hop, -(-s // hop)))
    m = sorted(k for k in m if 0 <= k < f)
    rng = np.random.default_rng([n, hop, t])
    if len(m) > limit // 2:
        m = list(rng.choice(m, limit // 2, replace=False))
    extra = rng.choice(f, limit - len(m), replace=False)
    return np.unique(np.concatenate([np.asarray(m, dtype=np.int64), extra]))


@functools.lru_cache(maxsize=None)
def reference(n, t, hop, win):
    """(frames, re, im) of direct() on signal(n, t) at the frames pick_frames() names."""
    fr = pick_frames(n, hop, t)
    re, im = direct(signal(n, t), n, bins_of(n), hop, win, fr)
    return fr, re, im


# The worst error of emulate() against direct() over every shape above (test_sdft_cpu.py measures it again and holds
# it to these), in units of u sqrt(N) max|x|; the device's bound is four times that: the errors are random-walk sums
# and a seed moves their maximum by about 2x (the margin test_gpu_stft_pair.py keeps over its measurements).  At
# N >= 1000 the bound stays below what order="sequential" gives over the same lengths at h = 1 (f32 13.2 / 35.2 / 69.5 u and
# f64 9.3 / 14.6 / 23.3 u at N = 1000 / 4096 / 16384; f64 at N = 1000 clears it by 5 % only): a device that scanned a
# chunk serially would miss it.
EMULATED_WORST = {"f32": 2.23, "f64": 2.21}
BOUND = {k: 4 * v for k, v in EMULATED_WORST.items()}


def err_units(got, re, im, n, dtype, xmax):
    """max |got - direct| / (u sqrt(N) max|x|): the metric of the bound (the windows' weights sum to 1 in magnitude)."""
    d = np.hypot(np.real(got).astype(LD) - re, np.imag(got).astype(LD) - im)
    return float(d.max() / (LD(U[dtype]) * np.sqrt(LD(n)) * LD(xmax)))


# ---- the path-by-path cases (test_sdft_exact_cpu.py, test_gpu_sdft_paths.py) ----------------------------------------

# N < E (2, 3, 5), the one-wave boundary (255 ... 257), f32's switch from E = 4 to E = 8 (1024 / 1025), the first second
# round (f64 1025, f32 2049: one live position in the last round), N not a multiple of E over several rounds (4097,
# 16383), f64's sixteenth round with one position (15361 = 15 x 1024 + 1) and the largest window.
PATH_SIZES = (2, 3, 5, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 15361, 16383, 16384)
PATH_WINDOWED = (3, 1025, 2049, 16384)
PATH_ROWS = 2


def path_lengths(n):
    return lengths(n) if n <= 2049 else (n, 2 * n + 1, 3 * n + 7)


def path_bins(n):
    return (0.0, 12.5, -3.0, n / 2)


def path_windows(n):
    return ("rect", "hann", "blackman") if n in PATH_WINDOWED else ("rect",)


def path_shape(n, win):
    """(rows, bins) of a case of the CPU test, which also computes long double references: two rows of four bins; one
    row of three where the emulation is slowest.  (The GPU test runs PATH_ROWS rows of path_bins everywhere.)"""
    if n == 16384 and win != "rect":
        return 1, path_bins(n)[:3]
    return PATH_ROWS, path_bins(n)


def rounds_of(n, dtype):
    """Rounds of 256 E positions per chunk."""
    return -(-n // (WG * segment(n, dtype)))


@functools.lru_cache(maxsize=8)
def emulated(n, t, win, dtype, rows, bins, seed=0):
    """emulate(exact=True) at hop 1 on the first `rows` rows of signal(n, t, seed): the device's bits, frame by frame."""
    return emulate(signal(n, t, seed)[:rows], n, bins, 1, win, dtype, exact=True)

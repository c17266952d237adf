"""An instrumented Python-integer model of the NTT kernels (pdsp_goldilocks.h, pdsp_ntt_kernel.h): the field functions
with the header's branch structure, counting per (site, branch) how often each conditional correction fired, and the
data flow of ntt_kernel<LOG2N, OP> step by step, every step with its inverse, so that a chosen state in front of any
step can be solved back to the input row that produces it.

Not the reference: ntt_ref.py stays the reference of every equality on the device.  The model says which branches a
row drives inside which unrolled instance, and builds rows that drive the rare ones.  No part of the product.

Branches of reduce128 (lo + 2^64 hi mod p): "borrow" (lo < hh), "overflow" (t + m >= 2^64), "canon" (the final
conditional subtraction).  mul_pow2 adds "wrap_*" for the reduce128(0, x) of a shift of 64 or more; its last reduction
uses the plain names.  sub and add count "sub_borrow".

Sites (a tuple, the unrolled instance of the kernel's code):
  (name, "tw", v, pass, u, t)        the inter-pass product reg[v][u + t U] * w[t], t > 0, pass > 0
  (name, "bf", v, pass, lg, b, i)    ntt_butterfly's stage lg, pair (b + i, b + i + half): add, sub and the shift
  (name, "pow", pass, u, t)          CONV's product tree w[t] = w[t / 2] * w[t - t / 2]
  ("split", v, m) ("pre", v, m)      CONV's u0 = a0 + a1 and u1 = (a0 - a1) * w^n, n = tid + TP m, v = 0 (a) / 1 (b)
  ("pw", m) ("post", m)              CONV's point-wise product and S1 * w^-n
  ("scale", m) / ("scale", m, half)  the 2^(192 - log2 N) at the store (inverse / CONV's two stores)
name is "fwd" or "inv": the forward and inverse pass chains (CONV runs both); v is the transform of the NV side by side.
CONV's two halves (h = 0, 1) run one loop body, so they share their sites.
"""
import random
from collections import Counter

import ntt_ref
from ntt_ref import EPS, P

M64 = 2 ** 64 - 1
INV2 = (P + 1) // 2
FORWARD, INVERSE, CONV = 0, 1, 2
OPS = (FORWARD, INVERSE, CONV)


# ---- the field, branch by branch (pdsp_goldilocks.h) -----------------------------------------------------------------


MUTANT = None  # (site, branch): that one correction comes out wrong by one -- the subtly wrong kernel the rows must catch


def _hit(cnt, site, branch):
    """Counts the branch; 1 where the correction is to come out wrong by one (MUTANT), else 0."""
    if cnt is not None:
        cnt[(site, branch)] += 1
    return int(MUTANT is not None and MUTANT == (site, branch))


def sub(a, b, cnt=None, site=None):
    d = a - b
    if d < 0:
        d += 2 ** 64 - EPS + _hit(cnt, site, "sub_borrow")
    return d


def add(a, b, cnt=None, site=None):
    return sub(a, P - b, cnt, site)


def neg(a):
    return P - a if a else 0


def reduce128(lo, hi, cnt=None, site=None, tag=""):
    hh, hl = hi >> 32, hi & EPS
    t = lo - hh
    if t < 0:
        t += 2 ** 64 - EPS + _hit(cnt, site, tag + "borrow")
    m = (hl << 32) - hl
    r = t + m
    if r >> 64:
        r = (r & M64) + EPS - _hit(cnt, site, tag + "overflow")
        assert r <= M64
    if r >= P:
        r -= P - _hit(cnt, site, tag + "canon")
    return r


def mul(a, b, cnt=None, site=None):
    w = a * b
    return reduce128(w & M64, w >> 64, cnt, site)


def mul_pow2(x, s, cnt=None, site=None):
    if s >= 96:
        x, s = neg(x), s - 96
    if s >= 64:
        x, s = reduce128(0, x, cnt, site, "wrap_"), s - 64
    return reduce128((x << s) & M64, x >> (64 - s), cnt, site) if s else x


def shift_parts(s):
    """mul_pow2's path for the constant s: (negates, wraps, the last shift)."""
    n = s >= 96
    s -= 96 * n
    w = s >= 64
    return n, w, s - 64 * w


# ---- the kernel's shape ----------------------------------------------------------------------------------------------


def log2e_of(log2n, op):
    return 4 if op == CONV or log2n >= 11 else 3


def rows_per_workgroup(log2n, op):
    tp = (1 << log2n) >> log2e_of(log2n, op)
    return 1 if tp >= 64 else 64 // tp


def bitrev(i, bits):
    return _BITREV[bits][i]


_BITREV = [[int(format(i, f"0{bits}b")[::-1], 2) if bits else 0 for i in range(1 << bits)] for bits in range(5)]


def butterfly_shift(lg, i, inv):
    fs = (39 * i * (64 >> lg)) % 192
    return (192 - fs) % 192 if inv else fs


_tables = {}


def table(log2w):
    """w^e, e < W = 2^log2w.  The kernel folds e >= W / 2 as p - w^(e - W / 2): the same values."""
    if log2w not in _tables:
        w, t = ntt_ref.root(1 << log2w), [1]
        for _ in range((1 << log2w) - 1):
            t.append(t[-1] * w % P)
        _tables[log2w] = t
    return _tables[log2w]


class Chain:
    """ntt_passes<LOG2T, LOG2E, LOG2W, INV, NV, ROW, POW, 0> for one of the NV transforms, as a list of steps on a
    state x[pos]: pos = tid + TP m is what thread tid holds in reg[m].  Steps: ("tw", pass), ("bf", pass, lg),
    ("perm", pass) -- the bit reversal in registers and the exchange (or, last pass, the registers kept)."""

    def __init__(self, name, log2t, log2e, log2w, inv):
        self.name, self.log2t, self.log2e, self.log2w, self.inv = name, log2t, log2e, log2w, inv
        self.T, self.TP = 1 << log2t, (1 << log2t) >> log2e
        self.passes, self.steps, self._groups, self._sources, self._table = [], [], {}, {}, table(log2w)
        done = 0
        while done < log2t:
            p, r = len(self.passes), min(log2e, log2t - done)
            self.passes.append((done, r))
            if p:
                self.steps.append(("tw", p))
            self.steps += [("bf", p, lg) for lg in range(r, 0, -1)] + [("perm", p)]
            done += r

    def groups(self, p):
        """Per butterfly of pass p: (j, u, k, positions of v[0 ... R - 1], output positions of V[0 ... R - 1])."""
        if p not in self._groups:
            log2ns, log2r = self.passes[p]
            stride, out = self.T >> log2r, []
            for j in range(stride):
                k = j & ((1 << log2ns) - 1)
                j0 = ((j >> log2ns) << (log2ns + log2r)) + k
                out.append((j, j // self.TP, k, [j + t * stride for t in range(1 << log2r)],
                            [j0 + (t << log2ns) for t in range(1 << log2r)]))
            self._groups[p] = out
        return self._groups[p]

    def factor(self, p, k, t, inverse_of=False):
        """w[t] of a butterfly of pass p: omega_(Ns R)^(t k), on the inverse roots for INV."""
        log2ns, log2r = self.passes[p]
        W = 1 << self.log2w
        e = t * k * ((self.T >> (log2ns + log2r)) << (self.log2w - self.log2t))
        return self._table[(W - e) % W if self.inv != inverse_of else e % W]

    def apply(self, step, x, cnt=None, v=0):
        kind, p = step[0], step[1]
        log2ns, log2r = self.passes[p]
        if kind == "tw":
            for j, u, k, pos, _ in self.groups(p):
                for t in range(1, 1 << log2r):
                    x[pos[t]] = mul(x[pos[t]], self.factor(p, k, t), cnt, (self.name, "tw", v, p, u, t))
        elif kind == "bf":
            lg = step[2]
            half = 1 << (lg - 1)
            for j, u, k, pos, _ in self.groups(p):
                for b in range(0, 1 << log2r, 2 * half):
                    for i in range(half):
                        site = (self.name, "bf", v, p, lg, b, i)
                        a, c = x[pos[b + i]], x[pos[b + i + half]]
                        x[pos[b + i]] = add(a, c, cnt, site)
                        x[pos[b + i + half]] = mul_pow2(sub(a, c, cnt, site), butterfly_shift(lg, i, self.inv), cnt, site)
        else:
            x[:] = [x[s] for s in self.sources(p)]

    def sources(self, p):
        """The exchange of pass p as a gather: the state after it is [x[s] for s in sources(p)]."""
        if p not in self._sources:
            log2r = self.passes[p][1]
            src = [0] * self.T
            for j, u, k, pos, out in self.groups(p):
                for i in range(1 << log2r):
                    src[out[bitrev(i, log2r)]] = pos[i]
            self._sources[p] = src
        return self._sources[p]

    def unapply(self, step, x):
        kind, p = step[0], step[1]
        log2ns, log2r = self.passes[p]
        if kind == "tw":
            for j, u, k, pos, _ in self.groups(p):
                for t in range(1, 1 << log2r):
                    x[pos[t]] = x[pos[t]] * self.factor(p, k, t, inverse_of=True) % P
        elif kind == "bf":
            lg = step[2]
            half = 1 << (lg - 1)
            back = [pow(2, (192 - butterfly_shift(lg, i, self.inv)) % 192, P) for i in range(half)]
            for j, u, k, pos, _ in self.groups(p):
                for b in range(0, 1 << log2r, 2 * half):
                    for i in range(half):
                        s, d = x[pos[b + i]], x[pos[b + i + half]] * back[i] % P
                        x[pos[b + i]], x[pos[b + i + half]] = (s + d) * INV2 % P, (s - d) * INV2 % P
        else:
            y = list(x)
            for d, s in enumerate(self.sources(p)):
                y[s] = x[d]
            x[:] = y

    def quick(self, step, x):
        """The step's values in plain modular arithmetic (what apply computes; no branch is looked at)."""
        kind, p = step[0], step[1]
        if kind == "tw":
            for j, u, k, pos, _ in self.groups(p):
                for t in range(1, len(pos)):
                    x[pos[t]] = x[pos[t]] * self.factor(p, k, t) % P
        elif kind == "bf":
            lg = step[2]
            half = 1 << (lg - 1)
            tw = [pow(2, butterfly_shift(lg, i, self.inv), P) for i in range(half)]
            for j, u, k, pos, _ in self.groups(p):
                for b in range(0, len(pos), 2 * half):
                    for i in range(half):
                        a, c = x[pos[b + i]], x[pos[b + i + half]]
                        x[pos[b + i]], x[pos[b + i + half]] = (a + c) % P, (a - c) * tw[i] % P
        else:
            self.apply(step, x)

    def run(self, x, cnt=None, v=0, capture=None, at=None):
        """The whole chain on a copy of x; capture = {step index: None} is filled with the states in front of them.
        at: the one step to run branch by branch and count (the others by quick()); None: every step."""
        x = list(x)
        for idx, step in enumerate(self.steps):
            if capture is not None and idx in capture:
                capture[idx] = list(x)
            if at is None or idx == at:
                self.apply(step, x, cnt, v)
            else:
                self.quick(step, x)
        return x

    def solve(self, idx, state):
        """The chain's input that puts `state` in front of step idx (idx = len(steps): the chain's output)."""
        x = list(state)
        for step in reversed(self.steps[:idx]):
            self.unapply(step, x)
        return x

    def pow_tree(self, cnt):
        """CONV's w[t] = mul(w[t / 2], w[t - t / 2]): table values only, the same for every row."""
        for p, (log2ns, log2r) in enumerate(self.passes):
            if p == 0:
                continue
            for j, u, k, _, _ in self.groups(p):
                w = [None, self.factor(p, k, 1)]
                for t in range(2, 1 << log2r):
                    w.append(mul(w[t // 2], w[t - t // 2], cnt, (self.name, "pow", p, u, t)))
                    assert w[t] == self.factor(p, k, t)


_chains = {}


def chain(log2n, op, name=None):
    """FORWARD / INVERSE: the one chain.  CONV: name "fwd" / "inv", the N/2-point chains on the N-point table."""
    if op != CONV:
        name = "inv" if op == INVERSE else "fwd"
    key = (log2n, op, name)
    if key not in _chains:
        _chains[key] = (Chain(name, log2n - 1, 3, log2n, name == "inv") if op == CONV else
                        Chain(name, log2n, log2e_of(log2n, op), log2n, op == INVERSE))
    return _chains[key]


def canon_row(x, n):
    return [v % P for v in x] + [0] * (n - len(x))


def transform(log2n, op, x, cnt=None, at=None):
    """ntt_kernel<log2n, FORWARD / INVERSE> on one row of 64-bit patterns.  at: Chain.run's (the scale always counts)."""
    ch = chain(log2n, op)
    y = ch.run(canon_row(x, ch.T), cnt, at=at)
    if op == INVERSE:
        y = [mul_pow2(v, 192 - log2n, cnt, ("scale", pos // ch.TP)) for pos, v in enumerate(y)]
    return y


def convolve(log2n, a, b, out_len=None, cnt=None, at=None):
    """ntt_kernel<log2n, CONV> on one pair of rows: a_len = len(a), b_len = len(b).  cnt: one counter, or one per half
    (the post-twiddle and the scale count with the second).  at: per half, the (chain name, step) whose step alone runs
    branch by branch in the pass chains (everything outside them always does); None: every step."""
    n = 1 << log2n
    half, tp, tab = n // 2, n // 16, table(log2n)
    a, b = canon_row(a, n), canon_row(b, n)
    fwd, inv = chain(log2n, CONV, "fwd"), chain(log2n, CONV, "inv")
    cnts = cnt if isinstance(cnt, (list, tuple)) else (cnt, cnt)
    s = []
    for h, c in enumerate(cnts):
        xy = [[0] * half, [0] * half]
        for v, r in enumerate((a, b)):
            for i in range(half):
                if h == 0:
                    xy[v][i] = add(r[i], r[i + half], c, ("split", v, i // tp))
                else:
                    xy[v][i] = mul(sub(r[i], r[i + half], c, ("pre", v, i // tp)), tab[i], c, ("pre", v, i // tp))
        on = {"fwd": None, "inv": None} if at is None else {name: at[h][1] if at[h][0] == name else -1 for name in ("fwd", "inv")}
        fa, fb = fwd.run(xy[0], c, 0, at=on["fwd"]), fwd.run(xy[1], c, 1, at=on["fwd"])
        s.append(inv.run([mul(fa[i], fb[i], c, ("pw", i // tp)) for i in range(half)], c, at=on["inv"]))
    out, c = [0] * n, cnts[1]
    for i in range(half):
        c1 = mul(s[1][i], tab[(n - i) % n], c, ("post", i // tp))
        out[i] = mul_pow2(add(s[0][i], c1, c, ("scale", i // tp, 0)), 192 - log2n, c, ("scale", i // tp, 0))
        out[i + half] = mul_pow2(sub(s[0][i], c1, c, ("scale", i // tp, 1)), 192 - log2n, c, ("scale", i // tp, 1))
    return out[:n if out_len is None else out_len]


# ---- operands that take a chosen branch --------------------------------------------------------------------------------


def fires(fn, branch):
    cnt = Counter()
    fn(cnt)
    return cnt[(None, branch)] > 0


def craft_mul(w, branch, rng, budget=64):
    """v < p with mul(v, w) taking `branch` ("borrow" / "canon"), or None.
    canon: the result is below eps, so v = c / w for a small c.  borrow: the product's low word is below its top 32
    bits, so v = lo / w mod 2^64 for a small lo (w = 2^z w': lo a multiple of 2^z, the top z bits of v free)."""
    if branch == "canon":
        winv = pow(w, P - 2, P)
        c = rng.randrange(1, 1 << 16)
        for step in range(budget):
            v = (c + step) * winv % P
            if fires(lambda cnt: mul(v, w, cnt), branch):
                return v
        return None
    z = (w & -w).bit_length() - 1
    bits = 64 - z
    winv = pow(w >> z, -1, 1 << bits)
    for attempt in range(budget):
        lo = attempt // 8 if z else attempt  # an even factor leaves top bits free: several draws per low word
        v = (lo * winv) % (1 << bits) + (rng.randrange(1 << z) << bits)
        if v < P and fires(lambda cnt: mul(v, w, cnt), branch):
            return v
    return None


def mul_can(w, branch):
    """What a canonical v needs for mul(v, w) to take the branch.  borrow wants hh >= 1: v w >= 2^96 with v < 2^64,
    so w > 2^32 (just above it hh stays tiny and whether a low word falls under it depends on w: craft_mul says).
    canon wants a value in [p, 2^64) before it: w >= 2."""
    return w > 2 ** 32 if branch == "borrow" else w >= 2


def shift_branches(s):
    """The rare branches mul_pow2(x, s) can take on a canonical x (DESIGN 4.14 argues each exclusion):
    the last shift s' takes canon for any 0 < s' < 64 and borrow only for s' > 32 (hi < 2^s', so hh = 0 up to 32);
    a wrap takes wrap_canon."""
    _, w, last = shift_parts(s)
    return (("canon",) if last else ()) + (("borrow",) if last > 32 else ()) + (("wrap_canon",) if w else ())


def craft_shift(s, branch, rng, budget=64):
    """x < p with mul_pow2(x, s) taking `branch`, or None."""
    n, w, last = shift_parts(s)
    if branch not in shift_branches(s):
        return None
    for step in range(budget):
        if branch == "wrap_canon":  # reduce128(0, hh 2^32 + 1) = p - hh + eps before the canon, 1 <= hh < eps
            x = (rng.randrange(1, EPS) << 32) + 1
        else:
            if branch == "borrow":  # x' = k 2^(64 - s'), k >= 2^32: a zero low word under a non-zero hh
                x = rng.randrange(1 << 32, 1 << last) << (64 - last)
            else:  # the result is below eps: x' = c 2^-s'
                x = (rng.randrange(1, 1 << 16) + step) * pow(2, 192 - last, P) % P
            if x >= P:
                continue
            if w:
                x = x * pow(2, 192 - 64, P) % P
        if n:
            x = neg(x)
        if fires(lambda cnt: mul_pow2(x, s, cnt), branch):
            return x
    return None


# ---- rows that drive a chosen step -------------------------------------------------------------------------------------


def uniform(rng, n):
    return [rng.randrange(P) for _ in range(n)]


def craft_state(ch, idx, branch, rng):
    """A state in front of step idx of the chain in which every operand of the step that can take `branch` does:
    (state, {site without name and v: crafted operands})."""
    step = ch.steps[idx]
    p = step[1]
    log2ns, log2r = ch.passes[p]
    x, owned = uniform(rng, ch.T), Counter()
    if step[0] == "tw":
        for j, u, k, pos, _ in ch.groups(p):
            for t in range(1, 1 << log2r):
                w = ch.factor(p, k, t)
                if mul_can(w, branch):
                    v = craft_mul(w, branch, rng)
                    if v is not None:
                        x[pos[t]] = v
                        owned[("tw", p, u, t)] += 1
    elif step[0] == "bf":
        lg = step[2]
        half = 1 << (lg - 1)
        for j, u, k, pos, _ in ch.groups(p):
            for b in range(0, 1 << log2r, 2 * half):
                for i in range(half):
                    d = craft_shift(butterfly_shift(lg, i, ch.inv), branch, rng)
                    if d is not None:
                        x[pos[b + i]] = (d + x[pos[b + i + half]]) % P
                        owned[("bf", p, lg, b, i)] += 1
    return x, owned


def step_targets(ch):
    """(step index, branch) for every step of the chain and every rare branch one of its instances can take."""
    out = []
    for idx, step in enumerate(ch.steps):
        if step[0] == "tw":
            out += [(idx, "borrow"), (idx, "canon")]
        elif step[0] == "bf":
            reach = {br for i in range(1 << (step[2] - 1)) for br in shift_branches(butterfly_shift(step[2], i, ch.inv))}
            out += [(idx, br) for br in ("borrow", "canon", "wrap_canon") if br in reach]
    return out


def transform_row_count(log2n, op):
    return len(step_targets(chain(log2n, op))) + (len(shift_branches(192 - log2n)) if op == INVERSE else 0)


def transform_rows(log2n, op, seed=0, only=None):
    """The branch rows of a forward or inverse transform: [(label, row, {branch: {site: crafted operands}})]; `only`:
    the indices to build (a row depends on its own seed alone)."""
    ch = chain(log2n, op)
    out, targets = [], step_targets(ch)
    for r, (idx, branch) in enumerate(targets):
        if only is not None and r not in only:
            continue
        rng = random.Random(f"{log2n} {op} {idx} {branch} {seed}")
        state, owned = craft_state(ch, idx, branch, rng)
        sites = {(ch.name, k[0], 0) + k[1:]: v for k, v in owned.items()}
        out.append((ch.steps[idx] + (branch,), ch.solve(idx, state), {branch: sites}))
    if op == INVERSE:
        for r, branch in enumerate(shift_branches(192 - log2n), len(targets)):
            if only is not None and r not in only:
                continue
            rng = random.Random(f"{log2n} scale {branch} {seed}")
            state = [craft_shift(192 - log2n, branch, rng) for _ in range(ch.T)]
            out.append((("scale", branch), ch.solve(len(ch.steps), state), {branch: {("scale", m): ch.TP for m in range(ch.T // ch.TP)}}))
    return out


def conv_targets(log2n):
    """The targets of one half of CONV that either half can take, then the ones of h = 1 alone, then the whole row's."""
    fwd, inv = chain(log2n, CONV, "fwd"), chain(log2n, CONV, "inv")
    either = [("fwd", idx, br) for idx, br in step_targets(fwd)] + [("pw", None, "borrow"), ("pw", None, "canon")]
    either += [("inv", idx, br) for idx, br in step_targets(inv)]
    second = [(k, None, br) for k in ("pre", "post") for br in ("borrow", "canon")]
    whole = [("scale", None, br) for br in shift_branches(192 - log2n)]
    return either, second, whole


def _spectra_for_product(c, rng):
    """Spectra a, b with a[i] b[i] = c[i]."""
    a = [rng.randrange(2, P) for _ in c]
    return a, [v * pow(u, -1, P) % P for u, v in zip(a, c)]


def conv_half(log2n, h, target, rng):
    """(u_h(a), u_h(b), {site: crafted operands}) for one half driven at `target` ((kind, step, branch) or None)."""
    n = 1 << log2n
    half, tp, tab = n // 2, n // 16, table(log2n)
    fwd, inv = chain(log2n, CONV, "fwd"), chain(log2n, CONV, "inv")
    sites = Counter()
    if target is None:
        return uniform(rng, half), uniform(rng, half), sites
    kind, idx, branch = target
    if kind == "fwd":
        us = []
        for v in range(2):
            state, owned = craft_state(fwd, idx, branch, rng)
            us.append(fwd.solve(idx, state))
            sites.update({("fwd", k[0], v) + k[1:]: c for k, c in owned.items()})
        return us[0], us[1], sites
    if kind == "pre":
        assert h == 1
        us = []
        for v in range(2):
            u = uniform(rng, half)
            for i in range(half):
                d = craft_mul(tab[i], branch, rng) if mul_can(tab[i], branch) else None
                if d is not None:
                    u[i] = d * tab[i] % P
                    sites[("pre", v, i // tp)] += 1
            us.append(u)
        return us[0], us[1], sites
    if kind == "pw":
        fb = [rng.randrange(2 ** 33, P) for _ in range(half)]
        fa = [craft_mul(w, branch, rng) for w in fb]
        for i in range(half):
            sites[("pw", i // tp)] += 1
    else:
        if kind == "inv":
            state, owned = craft_state(inv, idx, branch, rng)
            c = inv.solve(idx, state)
            sites.update({("inv", k[0], 0) + k[1:]: v for k, v in owned.items()})
        else:
            assert kind == "post" and h == 1
            s1 = uniform(rng, half)
            for i in range(half):
                w = tab[(n - i) % n]
                v = craft_mul(w, branch, rng) if mul_can(w, branch) else None
                if v is not None:
                    s1[i] = v
                    sites[("post", i // tp)] += 1
            c = inv.solve(len(inv.steps), s1)
        fa, fb = _spectra_for_product(c, rng)
    return fwd.solve(len(fwd.steps), fa), fwd.solve(len(fwd.steps), fb), sites


def conv_join(log2n, u0, u1):
    """The row whose decimation-in-frequency split is u0 = x0 + x1, u1 = (x0 - x1) w^n."""
    n = 1 << log2n
    tab = table(log2n)
    d = [u1[i] * tab[(n - i) % n] % P for i in range(n // 2)]
    return [(u0[i] + d[i]) * INV2 % P for i in range(n // 2)] + [(u0[i] - d[i]) * INV2 % P for i in range(n // 2)]


def conv_rows(log2n, seed=0, only=None):
    """The branch rows of CONV: [(label, a, b, [{branch: {site: crafted operands}} per half])].  A target either half
    can take is driven in h = 0 by row i and in h = 1 by row i + k of the first len(either) rows, k = ceil(len / 2), so
    the first k rows (conv_cover) drive every one of them once; then pre and post in h = 1, then the scale.  `only`: the
    indices to build."""
    n = 1 << log2n
    half, tp, tab = n // 2, n // 16, table(log2n)
    inv = chain(log2n, CONV, "inv")
    either, second, whole = conv_targets(log2n)
    k = (len(either) + 1) // 2
    pairs = [(either[i], either[(i + k) % len(either)]) for i in range(len(either))] + [(None, t) for t in second]
    out = []
    for r, (t0, t1) in enumerate(pairs):
        if only is not None and r not in only:
            continue
        rng = random.Random(f"{log2n} conv {t0} {t1} {seed}")
        ua0, ub0, s0 = conv_half(log2n, 0, t0, rng)
        ua1, ub1, s1 = conv_half(log2n, 1, t1, rng)
        expect = [{t[2]: s} if t is not None else {} for t, s in ((t0, s0), (t1, s1))]
        out.append(((t0, t1), conv_join(log2n, ua0, ua1), conv_join(log2n, ub0, ub1), expect))
    for r, (_, _, branch) in enumerate(whole, len(pairs)):
        if only is not None and r not in only:
            continue
        rng = random.Random(f"{log2n} conv scale {branch} {seed}")
        z = [[craft_shift(192 - log2n, branch, rng) for _ in range(half)] for _ in range(2)]
        s0 = [(z[0][i] + z[1][i]) * INV2 % P for i in range(half)]
        s1 = [(z[0][i] - z[1][i]) * INV2 % P * tab[i] % P for i in range(half)]
        us = [[], []]
        for s in (s0, s1):
            fa, fb = _spectra_for_product(inv.solve(len(inv.steps), s), rng)
            fwd = chain(log2n, CONV, "fwd")
            us[0].append(fwd.solve(len(fwd.steps), fa))
            us[1].append(fwd.solve(len(fwd.steps), fb))
        sites = {("scale", m, e): tp for m in range(8) for e in range(2)}
        out.append(((("scale", None, branch),), conv_join(log2n, *us[0]), conv_join(log2n, *us[1]), [{}, {branch: sites}]))
    return out


def conv_cover(log2n):
    """Indices of conv_rows that between them drive every target once: the large sizes' subset."""
    either, second, whole = conv_targets(log2n)
    total = len(either) + len(second) + len(whole)
    return list(range((len(either) + 1) // 2)) + list(range(len(either), total))


def rare(cnt):
    """{(site, branch): hits} of the rare branches alone: borrow and canon of a product or a last shift, wrap_canon."""
    return {k: v for k, v in cnt.items() if k[1] in ("borrow", "canon", "wrap_canon")}


def targeted_pairs(seed=0):
    """[(a, b, branch)]: canonical pairs whose product takes the borrow or the final canon of reduce128, for generic
    factors, table values, powers of two and their negatives; for ntt_mul_kernel and the host build of the header."""
    rng = random.Random(f"pairs {seed}")
    ws = [rng.randrange(2 ** 40, P) for _ in range(40)] + table(14)[1::1171] + [pow(2, j, P) for j in range(33, 192, 5)] + [2, 3, 8, 2 ** 32]
    out = []
    for w in ws:
        for branch in ("borrow", "canon"):
            v = craft_mul(w, branch, rng) if mul_can(w, branch) else None
            if v is not None:
                out += [(v, w, branch), (w, v, branch)]
    return out

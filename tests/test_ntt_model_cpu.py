"""The instrumented model of the NTT kernels (tests/ntt_model.py) on the CPU: the model computes what the reference
computes; its state solver puts a chosen state in front of any step; the rows the device tests had before never take
the borrow or the final canon of reduce128 in an inter-pass product; and the rows built here drive every rare branch in
every unrolled instance that can take it, at every size and op.  The device runs the same rows in
test_gpu_ntt_paths.py, against ntt_ref alone.

Pairs (site kind, branch) that no canonical operand can take -- the only ones the coverage condition leaves out:
  I1  a shift constant of 0 (i = 0 of every stage; all of stage 1): mul_pow2 returns x, no reduction runs.
  I2  borrow of a last shift s' <= 32: hi = x >> (64 - s') < 2^32, so hh = hi >> 32 = 0 and lo - hh never borrows.
      (The scale 2^(192 - log2 N) ends in s' = 18 ... 26: its last shift never borrows at any size.)
  I3  a product by the factor 1 (k = 0 of a pass; n = 0 of CONV's pre- and post-twiddle): hi = 0, r = lo = v < p.
  I4  borrow of a product by a factor w <= 2^32: v w < 2^64 2^32, so hi < 2^32 and hh = 0.  (Just above 2^32 hh stays tiny and
      the builder reports what it reached; the instance-level condition below does not depend on it.)
  I5  canon after an overflow, anywhere: r = t + m - p <= (2^64 - 1) + (2^32 - 1)^2 - p < p.
Not rare, so not part of the condition: sub_borrow, overflow, and the borrow of a wrap (reduce128(0, x) borrows for
every x >= 2^32)."""
import random
from collections import Counter

import pytest

import ntt_model as M
import ntt_ref
from ntt_ref import EPS, P

SIZES = range(6, 15)


def pairs_check(got, expect, where):
    for branch, sites in expect.items():
        for site, n in sites.items():
            assert got.get((site, branch), 0) == n, (where, site, branch, got.get((site, branch), 0), n)


# ---- the model is the kernels' arithmetic --------------------------------------------------------------------------------


def test_field_functions_equal_python_integers_on_corners_and_seeded_pairs():
    rng = random.Random(1)
    vals = sorted({v % P for v in ntt_ref.CORNERS}) + [rng.randrange(P) for _ in range(200)]
    for a in vals:
        for b in vals[:40]:
            assert M.mul(a, b) == a * b % P and M.add(a, b) == (a + b) % P and M.sub(a, b) == (a - b) % P
        for s in range(192):
            assert M.mul_pow2(a, s) == a * pow(2, s, P) % P, (a, s)


def test_the_recipes_reach_the_branches_and_the_exclusions_never_fire():
    rng = random.Random(2)
    edge = [0, 1, 2, EPS - 1, EPS, EPS + 1, 2 ** 32 + 1, 2 ** 63, P - 2, P - 1] + [k << s for s in (16, 31, 32, 33, 48) for k in (1, 3, EPS)]
    edge = [v for v in edge if v < P] + [rng.randrange(P) for _ in range(300)]
    for s in range(1, 192):
        reach = M.shift_branches(s)
        for branch in ("borrow", "canon", "wrap_canon"):
            x = M.craft_shift(s, branch, rng)
            assert (x is not None) == (branch in reach), (s, branch)  # every pair not excluded by I2 is reached
        cnt = Counter()
        for v in edge:
            M.mul_pow2(v, s, cnt)
        assert all(k[1] in reach or k[1] not in ("borrow", "canon", "wrap_canon") for k in cnt), (s, cnt)  # I2
    plain = [2, 3, 8, 2 ** 32, 2 ** 33, 2 ** 40 + 1, 2 ** 48, 2 ** 63] + [rng.randrange(2 ** 40, P) for _ in range(300)]
    for w in plain + [P - 1, P - 2, P - 2 ** 32] + M.table(6):  # the last: the negatives of powers of two, every factor at N = 64
        for branch in ("borrow", "canon"):
            v = M.craft_mul(w, branch, rng)
            assert v is None or M.mul_can(w, branch), (w, branch)  # I3, I4: the recipes find nothing where nothing is
            assert v is not None or w not in plain or not M.mul_can(w, branch), (w, branch)
        cnt = Counter()
        for v in edge:
            M.mul(v, w, cnt)
            M.mul(v, 1, cnt, "one")
        assert M.mul_can(w, "borrow") or cnt[(None, "borrow")] == 0  # I4
        assert not any(k[0] == "one" for k in cnt)  # I3


@pytest.mark.parametrize("log2n", SIZES)
def test_model_equals_the_reference(log2n):
    """Forward, inverse and CONV (cyclic and at partial lengths) on seeded rows of every kind."""
    n = 1 << log2n
    xs = ntt_ref.rows(n, len(ntt_ref.KINDS), 0, seed=41)
    for x in xs:
        assert M.transform(log2n, M.FORWARD, x) == ntt_ref.fast(x)
        assert M.transform(log2n, M.INVERSE, x) == ntt_ref.fast(x, inverse=True)
    for (i, j), (la, lb, lo) in zip(((0, 4), (1, 0), (3, 2)), ((n, n, n), (n - 3, 5, n - 3), (n // 2 - 1, n // 2 + 1, 7))):
        if log2n >= 12 and la == n - 3:
            continue  # a reference convolution costs three transforms: two lengths at the large sizes
        assert M.convolve(log2n, xs[i][:la], xs[j][:lb], lo) == ntt_ref.cyclic(xs[i][:la], xs[j][:lb], n)[:lo]


def chains():
    for log2n in (6, 7, 9, 11):
        for op in (M.FORWARD, M.INVERSE):
            yield M.chain(log2n, op)
    for log2n in (6, 7, 10):
        for name in ("fwd", "inv"):
            yield M.chain(log2n, M.CONV, name)


def test_solve_puts_a_chosen_state_in_front_of_every_step():
    rng = random.Random(3)
    for ch in chains():
        for idx in range(len(ch.steps) + 1):
            state = M.uniform(rng, ch.T)
            capture = {idx: None}
            out = ch.run(ch.solve(idx, state), capture=capture)
            assert (capture[idx] if idx < len(ch.steps) else out) == state, (ch.name, ch.log2t, idx)


@pytest.mark.parametrize("log2n,op", [(6, M.FORWARD), (9, M.INVERSE), (11, M.FORWARD), (12, M.INVERSE)])
def test_state_in_front_of_a_pass_is_the_sub_transforms_of_the_decimated_rows(log2n, op):
    """After passes whose radices multiply to Ns, position q Ns + k holds bin k of the Ns-point transform of
    x[q + (N / Ns) n]: the statement the rows could also be solved from, held to the model."""
    ch = M.chain(log2n, op)
    x = [v % P for v in ntt_ref.rows(ch.T, 1, 0, seed=5)[0]]
    capture = {idx: None for idx, step in enumerate(ch.steps) if step[0] == "tw"}
    ch.run(x, capture=capture)
    for idx, state in capture.items():
        ns = 1 << ch.passes[ch.steps[idx][1]][0]
        scale = pow(ns, P - 2, P) if op == M.INVERSE else 1  # fast() scales its inverse; the kernel scales once, at the store
        for q in range(ch.T // ns):
            got = [v * scale % P for v in state[q * ns:(q + 1) * ns]]
            assert got == ntt_ref.fast(x[q::ch.T // ns], inverse=op == M.INVERSE), (idx, q)


# ---- the gap: what the rows of test_gpu_ntt.py drive -------------------------------------------------------------------

POW2 = {pow(2, j, P) for j in range(192)}


def old_rows(log2n):
    """The distinct rows test_gpu_ntt.py puts through forward at this size, each with its kind (its inverse runs on
    their spectra, and on the rows of start 0 themselves)."""
    n = 1 << log2n
    calls = [(1, s) for s in (range(5) if log2n < 12 else (0,))] + [(3, s) for s in (0, 3, 4, 1)]
    if log2n < 12:
        calls += [(67, 0), (67, 3)]
    seen, out = set(), []
    for batch, start in calls:
        for r, x in enumerate(ntt_ref.rows(n, batch, start)):
            if tuple(x) not in seen:
                seen.add(tuple(x))
                out.append((ntt_ref.KINDS[(start + r) % len(ntt_ref.KINDS)], x))
    return out if log2n < 10 else out[:24]  # the later ones are more uniform and corner rows of the same making


@pytest.mark.parametrize("log2n", SIZES)
def test_baseline_the_old_rows_never_take_a_rare_branch_in_an_inter_pass_product(log2n):
    """Counted operand by operand, in front of every inter-pass product of forward (on the rows) and inverse (on their
    spectra, as test_gpu_ntt.py runs it): 0 borrows and 0 final canons at every site (pass, u, t) over the uniform
    rows, for the operands whose factor is not plus or minus a power of two.  Where the claim is dropped, and why:
      - factors 2^j (every factor at N = 64, where nothing is left of the claim; elsewhere the exponents that are
        multiples of N / 64): the product is a shift, its low word is zero for one operand in 2^(64 - j) (j = 60: one
        in 16), so the borrow is not rare there and uniform rows take it;
      - the structured rows (all p - 1, all 2^64 - 1, alternating, corners): their spectra are sparse or small, and the
        last pass of the inverse works on values that are about to become the small structured row again, so
        products come back below eps and the final canon fires at those sites (tens of hits per site); the borrow
        fires once or twice in all.  Some lanes of some instances, mostly of the inverse's last pass.
    Both sets of counts are printed (NTTBASE size chain pass u t branch power-of-two-factor uniform-row hits)."""
    tally = Counter()
    for op in (M.FORWARD, M.INVERSE):
        ch = M.chain(log2n, op)
        for kind, x in old_rows(log2n):
            x = [v % P for v in x] if op == M.FORWARD else ntt_ref.transform_rows([x])[0]
            capture = {idx: None for idx, step in enumerate(ch.steps) if step[0] == "tw"}
            ch.run(x, capture=capture)
            for idx, state in capture.items():
                p = ch.steps[idx][1]
                for j, u, k, pos, _ in ch.groups(p):
                    for t in range(1, len(pos)):
                        w, cnt = ch.factor(p, k, t), Counter()
                        M.mul(state[pos[t]], w, cnt)
                        for (_, branch), hits in cnt.items():
                            tally[(ch.name, p, u, t, branch, w in POW2, kind == "uniform")] += hits
    for key, hits in sorted(tally.items()):
        if key[4] in ("borrow", "canon"):
            print("NTTBASE", log2n, *key, hits)
    assert sum(1 for k in tally if k[4] == "overflow" and k[6]) > 0  # the tally sees the common branch
    assert [k for k in tally if k[4] in ("borrow", "canon") and not k[5] and k[6]] == []
    assert log2n == 6 or any(not k[5] and k[6] for k in tally)  # above N = 64 the claim is about something


# ---- the rows that close it --------------------------------------------------------------------------------------------


def instances(ch, v=0):
    """{(site, branch)} every instance of the chain's products and shifts can take (I1 ... I4 applied)."""
    out = set()
    for step in ch.steps:
        p = step[1]
        if step[0] == "tw":
            for j, u, k, pos, _ in ch.groups(p):
                for t in range(1, len(pos)):
                    out |= {((ch.name, "tw", v, p, u, t), br) for br in ("borrow", "canon") if M.mul_can(ch.factor(p, k, t), br)}
        elif step[0] == "bf":
            lg = step[2]
            for b in range(0, 1 << ch.passes[p][1], 1 << lg):
                for i in range(1 << (lg - 1)):
                    out |= {((ch.name, "bf", v, p, lg, b, i), br) for br in M.shift_branches(M.butterfly_shift(lg, i, ch.inv))}
    return out


def report(log2n, op, driven):
    kinds = Counter()
    for (site, branch), hits in driven.items():
        if site[0] in ("fwd", "inv"):  # the chain, the pass and, for a shift, the stage
            kind = f"{site[0]}.{site[1]}.pass{site[3]}" + (f".stage{site[4]}" if site[1] == "bf" else "")
        else:
            kind = site[0]
        kinds[(kind, branch)] += hits
    for (kind, branch), hits in sorted(kinds.items()):
        print("NTTCOV", log2n, ("forward", "inverse", "conv")[op], kind, branch, hits)


@pytest.mark.parametrize("op", (M.FORWARD, M.INVERSE))
@pytest.mark.parametrize("log2n", SIZES)
def test_branch_rows_drive_every_instance_of_a_transform(log2n, op):
    """Per row, the model's count at every instance of the driven step equals the operands crafted for it (every lane
    whose factor or constant can take the branch); over the rows, every (instance, rare branch) not excluded by
    I1 ... I4 is driven, every stage of every pass densely: no pair is left to a search."""
    ch = M.chain(log2n, op)
    driven = Counter()
    for label, row, expect in M.transform_rows(log2n, op):
        cnt = Counter()
        # below N = 1024 every step runs branch by branch; from there, the driven step does and the others run as plain
        # modular arithmetic (the same values: test_model_equals_the_reference runs every step of every size)
        M.transform(log2n, op, row, cnt, at=None if log2n < 10 else ch.steps.index(label[:-1]) if label[0] != "scale" else -1)
        pairs_check(cnt, expect, (log2n, op, label))
        for branch, sites in expect.items():
            for site, n in sites.items():
                driven[(site, branch)] += n
    want = instances(ch)
    if op == M.INVERSE:
        want |= {(("scale", m), br) for m in range(1 << ch.log2e) for br in M.shift_branches(192 - log2n)}
    assert {k for k, n in driven.items() if n > 0} == want
    # every unrolled instance of a product (pass >= 1, t > 0) takes both branches, but for one: the forward pass 1 on
    # 8 points per thread has the factors w_64^(5 k) = 2^(3 k), k < 8, at t = 5, all below 2^32: no borrow (I4)
    products = {(ch.name, "tw", 0, p, u, t) for p, (ns, r) in enumerate(ch.passes) if p for u in range((1 << ch.log2e) >> r) for t in range(1, 1 << r)}
    small = {("fwd", "tw", 0, 1, 0, 5)} if op == M.FORWARD and ch.log2e == 3 else set()
    assert {s for s, br in want if s[1] == "tw" and br == "canon"} == products
    assert {s for s, br in want if s[1] == "tw" and br == "borrow"} == products - small
    report(log2n, op, driven)


@pytest.mark.parametrize("log2n", SIZES)
def test_branch_rows_drive_every_instance_of_the_convolution(log2n):
    """The same for CONV, half by half (one loop body runs both halves, so a site driven in either is driven): the
    forward passes of a's and b's halves, the point-wise product, the inverse passes, the pre- and post-twiddle and both
    scales.  At N >= 4096 the rows are the subset that drives every target once (conv_cover)."""
    n, tp = 1 << log2n, (1 << log2n) // 16
    keep = None if log2n < 12 else set(M.conv_cover(log2n))
    driven = Counter()
    for label, a, b, expect in M.conv_rows(log2n, only=keep):
        cnts = [Counter(), Counter()]
        # from N = 1024 the driven steps alone run branch by branch, as in the transforms' test
        at = None if log2n < 10 else [t[:2] if t is not None and t[0] in ("fwd", "inv") else ("", -1) for t in (tuple(label) + (None,))[:2]]
        M.convolve(log2n, a, b, cnt=cnts, at=at)
        for h in range(2):
            pairs_check(cnts[h], expect[h], (log2n, label, h))
            for branch, sites in expect[h].items():
                for site, k in sites.items():
                    driven[(site, branch)] += k
    fwd, inv = M.chain(log2n, M.CONV, "fwd"), M.chain(log2n, M.CONV, "inv")
    want = instances(fwd, 0) | instances(fwd, 1) | instances(inv, 0)
    want |= {((kind, v, m), br) for kind in ("pre",) for v in range(2) for m in range(8) for br in ("borrow", "canon")}
    want |= {((kind, m), br) for kind in ("pw", "post") for m in range(8) for br in ("borrow", "canon")}
    want |= {(("scale", m, e), br) for m in range(8) for e in range(2) for br in M.shift_branches(192 - log2n)}
    assert {k for k, c in driven.items() if c > 0} == want
    assert driven[(("pw", 0), "borrow")] >= tp and driven[(("pre", 1, 1), "canon")] == tp
    report(log2n, M.CONV, driven)


@pytest.mark.parametrize("log2n", (6, 7, 9))
def test_every_branch_row_catches_its_correction_gone_wrong(log2n, monkeypatch):
    """The subtly wrong kernel: one correction (the borrow's - eps, the canon's - p) off by one in one unrolled
    instance, wherever that instance takes the branch.  For every row and every instance it drives, the model with
    that fault no longer equals the reference: an equality test on that row fails for that kernel.  (A canon merely
    left out is not the fault to ask for: the value stays right mod p and later arithmetic may forgive it.)"""
    for op in (M.FORWARD, M.INVERSE):
        for label, row, expect in M.transform_rows(log2n, op):
            want = ntt_ref.fast(row, inverse=op == M.INVERSE)
            assert M.transform(log2n, op, row, Counter()) == want
            for branch, sites in expect.items():
                for site in sites:
                    monkeypatch.setattr(M, "MUTANT", (site, branch))
                    assert M.transform(log2n, op, row, Counter()) != want, (log2n, op, label, site)
                    monkeypatch.setattr(M, "MUTANT", None)
    if log2n > 7:
        return
    for label, a, b, expect in M.conv_rows(log2n):
        want = ntt_ref.cyclic(a, b, 1 << log2n)
        for sites_of in expect:
            for branch, sites in sites_of.items():
                for site in sites:
                    monkeypatch.setattr(M, "MUTANT", (site, branch))
                    assert M.convolve(log2n, a, b, cnt=Counter()) != want, (log2n, label, site)
                    monkeypatch.setattr(M, "MUTANT", None)


@pytest.mark.parametrize("log2n", SIZES)
def test_pow_tree_branches_are_the_tables_own(log2n):
    """CONV's w[t] = w[t / 2] w[t - t / 2] multiplies table values: no input reaches it.  Printed, not driven."""
    for name in ("fwd", "inv"):
        cnt = Counter()
        M.chain(log2n, M.CONV, name).pow_tree(cnt)
        kinds = Counter()
        for (site, branch), hits in cnt.items():
            kinds[branch] += hits
        print("NTTPOW", log2n, name, dict(kinds))

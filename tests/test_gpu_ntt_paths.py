"""The NTT kernels branch by branch and path by path, on the device, against Python integers (tests/ntt_ref.py) by
equality alone.  The rows come from tests/ntt_model.py, which test_ntt_model_cpu.py shows to drive the borrow and the
final canon of reduce128 (and the canon of a shift's wrap) in every unrolled instance that can take them: the
inter-pass products (pass, u, t), every stage of every butterfly (pass, stage, b, i), CONV's pre-twiddle, point-wise
product, post-twiddle and the scale at the store.  The model builds rows and is never what a result is compared with.
Then CONV's row paths: partial lengths at every size, rows at strides with live words in the gaps, shared and per-row
b, batches around a workgroup's rows, in place; the transforms at strides; ntt_mul's counts."""
import random
from collections import Counter

import numpy as np
import pytest
import torch

import ntt_model as M
import ntt_ref
import pragma_dsp_amd as pd
from ntt_ref import P
from test_gpu_ntt import DEV, SENTINEL, copy, dev, host

pytestmark = pytest.mark.gpu
SIZES = range(6, 15)

# ---- branch rows -------------------------------------------------------------------------------------------------------

ROW_SECONDS = {M.FORWARD: 0.3, M.INVERSE: 0.3, M.CONV: 1.0}  # building and the reference of one 16384-point row, about


def row_indices(log2n, op):
    """The rows of the model run on the device: all of them; CONV at N >= 4096 the ones that cover every target once."""
    if op != M.CONV:
        return list(range(M.transform_row_count(log2n, op)))
    either, second, whole = M.conv_targets(log2n)
    return list(range(len(either) + len(second) + len(whole))) if log2n < 12 else M.conv_cover(log2n)


def chunks(log2n, op):
    """The rows in runs of about two seconds of Python integers each."""
    idx = row_indices(log2n, op)
    per = max(1, int(2.0 / (ROW_SECONDS[op] * (1 << log2n) / 16384)))
    return [idx[i:i + per] for i in range(0, len(idx), per)]


BRANCH_CASES = [(l, op, c) for l in SIZES for op in M.OPS for c in range(len(chunks(l, op)))]


def with_uniform_rows(crafted, log2n, op, maker):
    """Crafted rows with uniform ones between them (every third row; one in all at N >= 4096), more rows than a
    workgroup holds and no whole number of workgroups: dead rows run beside crafted ones."""
    rows_wg = M.rows_per_workgroup(log2n, op)
    out = []
    for i, row in enumerate(crafted):
        out.append(row)
        if i % 2 == 1 and log2n < 12:
            out.append(maker(i))
    out.append(maker(len(crafted)))
    while len(out) <= rows_wg or len(out) % rows_wg == 0 and rows_wg > 1:
        out.append(maker(len(out)))
    return out


@pytest.mark.parametrize("log2n,op,chunk", BRANCH_CASES)
def test_branch_rows_equal_the_reference_out_of_place_and_in_place(log2n, op, chunk):
    n = 1 << log2n
    plan = pd.Ntt(n, DEV)
    only = set(chunks(log2n, op)[chunk])
    if op != M.CONV:
        crafted = [row for _, row, _ in M.transform_rows(log2n, op, only=only)]
        assert len(crafted) == len(only)
        xs = with_uniform_rows(crafted, log2n, op, lambda i: ntt_ref.rows(n, 1, 0, seed=1000 * chunk + i)[0])
        want = ntt_ref.transform_rows(xs, inverse=op == M.INVERSE)
        run = plan.inverse if op == M.INVERSE else plan.forward
        x = dev(xs)
        assert host(run(x)) == want
        assert host(x) == xs
        assert run(x, out=x) is x and host(x) == want
        return
    crafted = [(a, b) for _, a, b, _ in M.conv_rows(log2n, only=only)]
    assert len(crafted) == len(only)
    pairs = with_uniform_rows(crafted, log2n, op, lambda i: tuple(ntt_ref.rows(n, 2, 0, seed=1000 * chunk + i)))
    as_, bs = [p[0] for p in pairs], [p[1] for p in pairs]
    want = [ntt_ref.cyclic(a, b, n) for a, b in pairs]
    a, b = dev(as_), dev(bs)
    assert host(plan.convolve(a, b, out_len=n)) == want
    assert host(a) == as_ and host(b) == bs
    assert plan.convolve(a, b, out_len=n, out=a) is a and host(a) == want


def test_ntt_mul_takes_every_rare_branch_of_the_product():
    """Pairs built to take the borrow and the final canon (the model counts one hit of the named branch per pair),
    both ways round, among uniform pairs; out of place, out == a and out == b."""
    pairs = M.targeted_pairs()
    hits = Counter()
    for x, y, branch in pairs:
        cnt = Counter()
        M.mul(x, y, cnt)
        assert cnt[(None, branch)] == 1, (x, y, branch)
        hits[branch] += 1
    assert hits["borrow"] >= 100 and hits["canon"] >= 100
    rng = random.Random(9)
    both = [(x, y) for x, y, _ in pairs] + [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(77)]
    rng.shuffle(both)
    a, b = dev([p[0] for p in both]), dev([p[1] for p in both])
    want = [x * y % P for x, y in both]
    assert host(pd.ntt_mul(a, b)) == want
    a2, b2 = copy(a), copy(b)
    assert pd.ntt_mul(a2, b, out=a2) is a2 and host(a2) == want
    assert pd.ntt_mul(a, b2, out=b2) is b2 and host(b2) == want


# ---- row paths -----------------------------------------------------------------------------------------------------------


def pattern(i):
    """A non-zero 64-bit pattern >= p, different from word to word: what a gap of an input holds."""
    return P + 1 + (i * 2654435761) % (2 ** 32 - 2)


class Strided:
    """Rows of `length` words at a row stride of `stride`, from a base one word into the allocation, with three words
    behind the last row's stride; every word that is not a row's holds fill(i)."""

    def __init__(self, rows, length, stride, fill):
        self.batch, self.length, self.stride = len(rows), length, stride
        self.words = [fill(i) for i in range(1 + self.batch * stride + 3)]
        for r, row in enumerate(rows):
            assert len(row) == length <= stride
            self.words[1 + r * stride:1 + r * stride + length] = row
        self.flat = dev(self.words)

    def view(self, length=None):
        body = self.flat.view(torch.int64)[1:1 + self.batch * self.stride].view(self.batch, self.stride)
        return body[:, :self.length if length is None else length].view(torch.uint64)

    def expect(self, rows, length):
        """The words with `rows` (of `length` words) written over the rows' first words."""
        words = list(self.words)
        for r, row in enumerate(rows):
            words[1 + r * self.stride:1 + r * self.stride + length] = row
        return words


def batch_sizes(log2n, op):
    rows_wg = M.rows_per_workgroup(log2n, op)
    return (1, 3, 5) if rows_wg == 1 else (1, rows_wg - 1, rows_wg + 1, 2 * rows_wg + 3)


def conv_lengths(n):
    """(a_len, b_len, out_len): cyclic; the linear product that fills the row; one value; a short b; odd lengths with
    out_len < a_len; out_len > a_len."""
    return [(n, n, n), (n // 2, n // 2 + 1, n), (1, 1, 1), (n - 3, 5, n - 3), (n // 2 - 1, 9, n // 4 + 1), (n // 4 + 1, n // 2 - 3, n - 5)]


@pytest.mark.parametrize("case", range(6))
@pytest.mark.parametrize("log2n", SIZES)
def test_convolution_row_paths_equal_the_reference(log2n, case):
    """Every size at every length case, against ntt_ref.cyclic.  a, per-row b and out at row strides above their
    lengths from bases one word into their allocations: the gaps of a and b and the words behind their last rows hold
    non-zero patterns >= p (read as data, they would change the result), out's gaps and borders a sentinel (checked
    bit for bit), and a and b are checked unchanged.  Batches of 1, ROWS - 1, ROWS + 1 and 2 ROWS + 3 (ROWS = 1: 1, 3,
    5): the last workgroup has dead rows.  One shared b row (b_stride == 0) from an offset base.  In place (out == a at
    one stride >= both lengths) for the cases with out_len < a_len and out_len > a_len."""
    n = 1 << log2n
    plan = pd.Ntt(n, DEV)
    a_len, b_len, out_len = conv_lengths(n)[case]
    sizes = batch_sizes(log2n, M.CONV)
    as_ = [r[:a_len] for r in ntt_ref.rows(n, sizes[-1], 0, seed=17 + case)]
    bs = [r[:b_len] for r in ntt_ref.rows(n, sizes[-1], 2, seed=23 + case)]
    want = [ntt_ref.cyclic(as_[r], bs[r], n)[:out_len] for r in range(sizes[-1])]
    for batch in sizes:
        a = Strided(as_[:batch], a_len, a_len + 3, pattern)
        b = Strided(bs[:batch], b_len, b_len + 5, pattern)
        out = Strided([[SENTINEL] * out_len] * batch, out_len, out_len + 7, lambda i: SENTINEL)
        got = plan.convolve(a.view(), b.view(), out_len=out_len, out=out.view())
        assert host(got) == want[:batch], (n, case, batch)
        assert host(out.flat) == out.expect(want[:batch], out_len), (n, case, batch)
        assert host(a.flat) == a.words and host(b.flat) == b.words, (n, case, batch)
    # one shared b row, from an offset base, its neighbours live
    batch = sizes[2]
    shared = Strided([bs[0]], b_len, b_len + 5, pattern)
    a = Strided(as_[:batch], a_len, a_len + 1, pattern)
    want_shared = [want[0]] + [ntt_ref.cyclic(as_[r], bs[0], n)[:out_len] for r in range(1, batch)]
    got = plan.convolve(a.view(), shared.view()[0], out_len=out_len)
    assert host(got) == want_shared and host(shared.flat) == shared.words and host(a.flat) == a.words, (n, case)
    if out_len != a_len and a_len > 1:  # in place: out == a, one stride for both, the words past out_len left alone
        a = Strided([r + [pattern(7 * i) for i in range(max(out_len - a_len, 0))] for r in as_[:batch]],
                    max(a_len, out_len), max(a_len, out_len) + 3, pattern)
        b = Strided(bs[:batch], b_len, b_len + 2, pattern)
        assert host(plan.convolve(a.view(a_len), b.view(), out_len=out_len, out=a.view(out_len))) == want[:batch]
        assert host(a.flat) == a.expect(want[:batch], out_len) and host(b.flat) == b.words, (n, case)


@pytest.mark.parametrize("log2n", SIZES)
def test_transforms_at_odd_strides_from_offset_bases(log2n):
    """forward and inverse with input and output both at odd row strides from bases one word in, live patterns >= p in
    the input's gaps, a sentinel in the output's, at batches around a workgroup's rows."""
    n = 1 << log2n
    plan = pd.Ntt(n, DEV)
    sizes = batch_sizes(log2n, M.FORWARD)
    xs = ntt_ref.rows(n, sizes[-1], 1, seed=29)
    for inverse, run in ((False, plan.forward), (True, plan.inverse)):
        want = ntt_ref.transform_rows(xs, inverse=inverse)
        for batch in sizes:
            x = Strided(xs[:batch], n, n + 3, pattern)
            out = Strided([[SENTINEL] * n] * batch, n, n + 5, lambda i: SENTINEL)
            assert host(run(x.view(), out=out.view())) == want[:batch], (n, inverse, batch)
            assert host(out.flat) == out.expect(want[:batch], n) and host(x.flat) == x.words, (n, inverse, batch)


def test_ntt_mul_counts_around_a_workgroup_and_beyond_one_sweep_of_the_grid():
    """Counts 1, 255, 257 and 2048 * 256 + 257: the launch caps its grid at 2048 workgroups of 256 (grid_for), so the
    last count makes every thread of the first 257 take a second element and the others stop.  out == b at each."""
    rng = np.random.default_rng(11)
    for count in (1, 255, 257, 2048 * 256 + 257):
        av = rng.integers(0, 2 ** 64, size=count, dtype=np.uint64, endpoint=False)
        bv = rng.integers(0, 2 ** 64, size=count, dtype=np.uint64, endpoint=False)
        want = [x * y % P for x, y in zip(av.tolist(), bv.tolist())]
        a = Strided([av.tolist()], count, count + 2, lambda i: SENTINEL)
        b = Strided([bv.tolist()], count, count + 2, lambda i: SENTINEL)
        out = Strided([[SENTINEL] * count], count, count + 2, lambda i: SENTINEL)
        assert host(pd.ntt_mul(a.view()[0], b.view()[0], out=out.view()[0])) == want, count
        assert host(out.flat) == out.expect([want], count) and host(a.flat) == a.words, count
        assert pd.ntt_mul(a.view()[0], b.view()[0], out=b.view()[0]).data_ptr() == b.view().data_ptr()
        assert host(b.flat) == b.expect([want], count) and host(a.flat) == a.words, count

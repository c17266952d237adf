"""The NTT over GF(2^64 - 2^32 + 1) on the device against Python integers (tests/ntt_ref.py): every size 2^6 ... 2^14
forward and inverse, the fused convolution against the definition's transforms and against its four-launch composition,
the element-wise product, the exact signed convolution and the host forms.  Every comparison is equality of 64-bit
integers; there is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

import ntt_ref
import pragma_dsp_amd as pd
from ntt_ref import CORNERS, P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0xDEADBEEFCAFEF00D


def dev(rows, dtype=torch.uint64):
    """Rows of Python integers -> a device tensor of uint64 (moved as int64, the same bits)."""
    a = np.array(rows, dtype=np.uint64)
    return torch.from_numpy(a.view(np.int64)).to(DEV).view(dtype)


def copy(t):
    return t.view(torch.int64).clone().view(t.dtype)


def host(t):
    """A device tensor of 64-bit words -> nested lists of Python integers."""
    return t.contiguous().view(torch.int64).cpu().numpy().view(np.uint64).tolist()


def batches(log2n):
    return (1, 3) if log2n >= 12 else (1, 3, 67)


CASES = [(l, b) for l in range(6, 15) for b in batches(l)]


@pytest.mark.parametrize("log2n,batch", CASES)
def test_forward_and_inverse_equal_the_reference(log2n, batch):
    """forward == reference, inverse(forward(x)) == x mod p, inverse == reference, on rows of every kind (uniform
    64-bit patterns with values >= p, all p - 1, all 2^64 - 1, alternating 0 / p - 1, corner values)."""
    n = 1 << log2n
    plan = pd.Ntt(n, DEV)
    assert plan.size == n
    # kinds of rows: a one-row call per kind at the small sizes; KINDS[0:3] and KINDS[3:5] + KINDS[0] in batches of three
    for start in (range(5) if log2n < 12 else (0,)) if batch == 1 else (0, 3):
        xs = ntt_ref.rows(n, batch, start)
        x = dev(xs)
        want = ntt_ref.transform_rows(xs)
        got = plan.forward(x)
        assert got.dtype == torch.uint64 and got.shape == x.shape
        assert host(got) == want, (n, batch, start)
        back = plan.inverse(got)
        assert host(back) == [[v % P for v in r] for r in xs], (n, batch, start)
        if start == 0:  # the inverse on rows that are nobody's spectrum, patterns >= p among them
            assert host(plan.inverse(x)) == ntt_ref.transform_rows(xs, inverse=True), (n, batch, start)


@pytest.mark.parametrize("log2n", range(6, 15))
def test_in_place_out_identity_and_int64(log2n):
    n = 1 << log2n
    plan = pd.Ntt(n, DEV)
    xs = ntt_ref.rows(n, 3, 4)
    want = ntt_ref.transform_rows(xs)
    x = dev(xs)
    out = torch.empty_like(x)
    assert plan.forward(x, out=out) is out and host(out) == want
    y = copy(x)
    assert plan.forward(y, out=y) is y and host(y) == want  # the exact in-place call
    assert plan.inverse(y, out=y) is y and host(y) == [[v % P for v in r] for r in xs]
    xi = dev(xs, torch.int64)
    gi = plan.forward(xi)
    assert gi.dtype == torch.int64 and host(gi) == want  # the same bits under either dtype
    x1 = dev(xs[0])  # one row, 1-D
    assert host(plan(x1)) == want[0]


@pytest.mark.parametrize("log2n", range(6, 15))
def test_rows_at_a_stride_leave_the_padding_alone(log2n):
    n, batch = 1 << log2n, 3
    plan = pd.Ntt(n, DEV)
    xs = ntt_ref.rows(n, batch, 1)
    want = ntt_ref.transform_rows(xs)
    for pad_in, pad_out in ((5, 0), (0, 3), (7, 7)):
        src = torch.full((batch, n + pad_in), SENTINEL - (1 << 64), dtype=torch.int64, device=DEV).view(torch.uint64)
        dst = torch.full((batch, n + pad_out), SENTINEL - (1 << 64), dtype=torch.int64, device=DEV).view(torch.uint64)
        src[:, :n].view(torch.int64).copy_(dev(xs).view(torch.int64))
        got = plan.forward(src[:, :n], out=dst[:, :n])
        assert host(got) == want
        assert all(v == SENTINEL for r in host(dst[:, n:]) for v in r) and all(v == SENTINEL for r in host(src[:, n:]) for v in r)
        assert host(src[:, :n]) == xs  # the input is untouched


def conv_shapes(n):
    return [(n, n, n), (n // 2, n // 2 + 1, n), (1, 1, 1), (n - 3, 5, n - 3)]


@pytest.mark.parametrize("n", [64, 128, 4096, 16384])
def test_convolution_equals_the_reference_and_the_composition(n):
    """(a_len, b_len, out_len): cyclic, the linear product that exactly fills the row, one value, a short b; per-row b
    and one shared b; against Python integers and against forward, forward, ntt_mul, inverse on the device."""
    plan = pd.Ntt(n, DEV)
    batch = 3
    for a_len, b_len, out_len in conv_shapes(n):
        as_ = [r[:a_len] for r in ntt_ref.rows(n, batch, 0, seed=a_len)]
        bs = [r[:b_len] for r in ntt_ref.rows(n, batch, 2, seed=b_len + 1)]
        a, b = dev(as_), dev(bs)
        for shared in (False, True):
            bb = b[0] if shared else b
            want = [ntt_ref.cyclic(as_[r], bs[0 if shared else r], n)[:out_len] for r in range(batch)]
            got = plan.convolve(a, bb, out_len=out_len)
            assert got.shape == (batch, out_len) and host(got) == want, (n, a_len, b_len, out_len, shared)
            # the four-launch composition on zero-padded rows
            az = torch.zeros((batch, n), dtype=torch.int64, device=DEV)
            bz = torch.zeros((batch, n), dtype=torch.int64, device=DEV)
            az[:, :a_len] = a.view(torch.int64)
            bz[:, :b_len] = (b[:1] if shared else b).view(torch.int64)
            comp = plan.inverse(pd.ntt_mul(plan.forward(az), plan.forward(bz)))
            assert torch.equal(comp[:, :out_len], got.view(torch.int64)), (n, a_len, b_len, out_len, shared)
    # default out_len: the linear product where it fits; out == a in place
    a, b = dev([r[:n // 2] for r in ntt_ref.rows(n, 2, 0)]), dev(ntt_ref.rows(n, 1, 4)[0][:9])
    full = plan.convolve(a, b)
    assert full.shape == (2, n // 2 + 8)
    a2 = copy(a)
    assert plan.convolve(a2, b, out_len=n // 2, out=a2) is a2 and torch.equal(a2.view(torch.int64), full[:, :n // 2].view(torch.int64))


@pytest.mark.parametrize("log2n", range(6, 15))
def test_cyclic_convolution_equals_the_composition_at_every_size(log2n):
    n = 1 << log2n
    plan = pd.Ntt(n, DEV)
    a, b = dev(ntt_ref.rows(n, 5, 0, seed=11)), dev(ntt_ref.rows(n, 5, 3, seed=12))
    comp = plan.inverse(pd.ntt_mul(plan.forward(a), plan.forward(b)))
    assert torch.equal(plan.convolve(a, b, out_len=n).view(torch.int64), comp.view(torch.int64))
    assert torch.equal(plan.convolve(a, b[2], out_len=n)[2].view(torch.int64), comp[2].view(torch.int64))


def test_ntt_mul_on_corner_pairs_and_a_ragged_count():
    pairs = [(a, b) for a in CORNERS for b in CORNERS]
    rng = np.random.default_rng(5)
    extra = rng.integers(0, 2 ** 64, size=(1000 + 3, 2), dtype=np.uint64, endpoint=False).tolist()
    pairs += [tuple(p) for p in extra]  # 1228 values: not a multiple of the workgroup's 256
    a, b = dev([p[0] for p in pairs]), dev([p[1] for p in pairs])
    want = [x * y % P for x, y in pairs]
    assert host(pd.ntt_mul(a, b)) == want
    ai = a.view(torch.int64).clone()
    assert pd.ntt_mul(ai, b.view(torch.int64), out=ai) is ai and host(ai) == want  # out == a, int64


@pytest.mark.parametrize("la,lb", [(1, 1), (100, 29), (2048, 2049), (8000, 8385), (3, 16382)])
def test_convolve_exact_equals_numpy_convolve(la, lb):
    """|values| < 2^20: sums of at most 2^14 products below 2^40 are exact in int64."""
    rng = np.random.default_rng(la * 31 + lb)
    a = rng.integers(-(2 ** 20) + 1, 2 ** 20, size=(2, la), dtype=np.int64)
    b = rng.integers(-(2 ** 20) + 1, 2 ** 20, size=lb, dtype=np.int64)
    got = pd.convolve_exact(a, b)
    assert got.dtype == np.int64 and got.shape == (2, la + lb - 1)
    for r in range(2):
        assert np.array_equal(got[r], np.convolve(a[r], b))
    assert np.array_equal(pd.convolve_exact(a[0], b), np.convolve(a[0], b))


@pytest.mark.parametrize("n", [64, 4096])
def test_host_forms_equal_the_reference_and_the_device(n):
    xs = ntt_ref.rows(n, 3, 0, seed=n)
    x = np.array(xs, dtype=np.uint64)
    want = ntt_ref.transform_rows(xs)
    got = pd.ntt(x)
    assert got.dtype == np.uint64 and got.tolist() == want
    assert pd.intt(got).tolist() == [[v % P for v in r] for r in xs]
    assert pd.ntt(x[0]).tolist() == want[0] and pd.ntt(x.view(np.int64)).tolist() == want
    assert got.tolist() == host(pd.Ntt(n, DEV).forward(dev(xs)))
    # polymul: the linear product on the next power of two
    la, lb = n // 2, n // 2 + 1
    a, b = x[:, :la], x[0, :lb]
    prod = pd.polymul(a, b)
    assert prod.shape == (3, n) and prod.tolist() == [ntt_ref.cyclic(xs[r][:la], xs[0][:lb], n) for r in range(3)]
    assert pd.polymul(a, x[:, :lb])[1].tolist() == ntt_ref.cyclic(xs[1][:la], xs[1][:lb], n)

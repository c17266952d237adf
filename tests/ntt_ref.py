"""The reference of the NTT tests, in Python integers alone: the field GF(p), p = 2^64 - 2^32 + 1, the root
w_N = 7^((p - 1) / N), the transform by its definition (O(N^2)) and an iterative radix-2 transform that
test_ntt_cpu.py pins to the definition at N = 64; the cyclic convolution by its definition and through the transforms;
the corner values and the seeded rows the tests run on.  Not the oracle, and no part of the product: nothing here is
imported by the package."""
import random

P = 2 ** 64 - 2 ** 32 + 1
EPS = 2 ** 32 - 1
GENERATOR = 7
CORNERS = [0, 1, 2, EPS - 1, EPS, EPS + 1, 2 ** 33, 2 ** 48, 2 ** 63, P - 2, P - 1, P, P + 1, 2 ** 64 - 2 ** 32, 2 ** 64 - 1]
KINDS = ("uniform", "p-1", "ones", "alternating", "corners")


def root(n):
    assert n >= 1 and n & (n - 1) == 0 and (P - 1) % n == 0
    return pow(GENERATOR, (P - 1) // n, P)


def direct(x, inverse=False):
    """X[k] = sum_n x[n] w^(n k) mod p; inverse: x[n] = N^-1 sum_k X[k] w^(-n k) mod p."""
    n = len(x)
    w = root(n)
    if inverse:
        w = pow(w, P - 2, P)
    pw = [pow(w, j, P) for j in range(n)]
    out = [sum(x[j] * pw[j * k % n] for j in range(n)) % P for k in range(n)]
    if inverse:
        ninv = pow(n, P - 2, P)
        out = [v * ninv % P for v in out]
    return out


def fast(x, inverse=False):
    """The same transform, iteratively: bit-reversed input, decimation-in-time stages of radix 2."""
    n = len(x)
    bits = n.bit_length() - 1
    a = [0] * n
    for i, v in enumerate(x):
        a[int(format(i, f"0{bits}b")[::-1], 2) if bits else 0] = v % P
    w = root(n)
    if inverse:
        w = pow(w, P - 2, P)
    size = 2
    while size <= n:
        half, step = size // 2, pow(w, n // size, P)
        tw = [1] * half
        for j in range(1, half):
            tw[j] = tw[j - 1] * step % P
        for s in range(0, n, size):
            for j in range(half):
                u, v = a[s + j], a[s + j + half] * tw[j] % P
                a[s + j], a[s + j + half] = (u + v) % P, (u - v) % P
        size *= 2
    if inverse:
        ninv = pow(n, P - 2, P)
        a = [v * ninv % P for v in a]
    return a


def cyclic_direct(a, b, n):
    """c[i] = sum_{j + l = i mod n} a[j] b[l] mod p by the definition; a and b zero-padded to n."""
    c = [0] * n
    for j, u in enumerate(a):
        for l, v in enumerate(b):
            c[(j + l) % n] = (c[(j + l) % n] + u * v) % P
    return c


def cyclic(a, b, n):
    """The same through the transforms (pinned to cyclic_direct in test_ntt_cpu.py)."""
    fa = fast(list(a) + [0] * (n - len(a)))
    fb = fast(list(b) + [0] * (n - len(b)))
    return fast([u * v % P for u, v in zip(fa, fb)], inverse=True)


def row(kind, n, rng):
    """One row of n 64-bit patterns: KINDS."""
    if kind == "uniform":
        return [rng.getrandbits(64) for _ in range(n)]
    if kind == "p-1":
        return [P - 1] * n
    if kind == "ones":
        return [2 ** 64 - 1] * n
    if kind == "alternating":
        return [0 if i % 2 == 0 else P - 1 for i in range(n)]
    if kind == "corners":
        return [rng.choice(CORNERS) for _ in range(n)]
    raise ValueError(kind)


def rows(n, batch, start=0, seed=0):
    """`batch` rows whose kinds cycle through KINDS from KINDS[start]; a uniform row holds a few patterns >= p for sure."""
    rng = random.Random(1000003 * n + 101 * batch + 7 * start + seed)
    out = []
    for r in range(batch):
        x = row(KINDS[(start + r) % len(KINDS)], n, rng)
        if KINDS[(start + r) % len(KINDS)] == "uniform":
            for _ in range(4):
                x[rng.randrange(n)] = rng.randrange(P, 2 ** 64)
        out.append(x)
    return out


_cache = {}


def transform_rows(xs, inverse=False):
    """fast() of every row, computed once per distinct row."""
    out = []
    for x in xs:
        key = (inverse, tuple(x))
        if key not in _cache:
            _cache[key] = fast(x, inverse)
        out.append(_cache[key])
    return out

#!/usr/bin/env python3
"""Daubechies' extremal-phase scaling filters db1 ... db10, as the f64 table of pragma-dsp_amd/csrc/pdsp_capi_dwt.hip
(kDaubechies).  numpy only.

For p vanishing moments: P(y) = sum_{k < p} C(p - 1 + k, k) y^k is the polynomial with
(1 - y)^p P(y) + y^p P(1 - y) = 1.  With y = (2 - z - 1/z) / 4, each root y0 of P gives the pair of roots
z, 1 / z of z^2 - (2 - 4 y0) z + 1; keeping the one inside the unit circle is the spectral factor of minimum
phase.  The filter is (1 + z)^p times the product of (z - z_i), normalised to sum sqrt(2).  In that order the first
taps are the large ones: db2 = [(1 + sqrt 3), (3 + sqrt 3), (3 - sqrt 3), (1 - sqrt 3)] / (4 sqrt 2).

The orthonormality residual max_m |sum_k h[k] h[k + 2m] - delta_m| of this construction is <= 1e-15 up to db10 and
degrades beyond it (the roots of P crowd together), which is why the table stops there.

    python tools/gen_daubechies.py            prints the C table
    python tools/gen_daubechies.py --check    prints each filter's residual
"""
import sys
from math import comb

import numpy as np

MAX_P = 10


def daubechies(p: int) -> np.ndarray:
    """The 2p taps of db<p>."""
    if p < 1:
        raise ValueError("p must be >= 1")
    zs = []
    if p > 1:
        coeffs = [comb(p - 1 + k, k) for k in range(p)]  # ascending in y
        for y0 in np.roots(coeffs[::-1]):
            b = 2.0 - 4.0 * y0
            d = np.sqrt(b * b - 4.0 + 0j)
            z1, z2 = (b + d) / 2.0, (b - d) / 2.0
            zs.append(z1 if abs(z1) < 1.0 else z2)
    h = np.poly(np.concatenate([-np.ones(p), np.asarray(zs, dtype=complex)]))
    h = np.real(h)
    return h * (np.sqrt(2.0) / h.sum())


def residual(h: np.ndarray) -> float:
    f = h.size
    return max(abs(float(np.dot(h[: f - 2 * m], h[2 * m:])) - (1.0 if m == 0 else 0.0)) for m in range(f // 2))


def table() -> str:
    lines = []
    for p in range(1, MAX_P + 1):
        h = daubechies(p)
        lines.append(f"    // db{p}")
        for i in range(0, h.size, 4):
            lines.append("    " + " ".join(f"{float(v)!r}," for v in h[i:i + 4]))
    return "\n".join(lines)


if __name__ == "__main__":
    if "--check" in sys.argv[1:]:
        for p in range(1, MAX_P + 1):
            print(f"db{p}: {2 * p} taps, residual {residual(daubechies(p)):.2e}")
    else:
        print(table())

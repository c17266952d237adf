"""ntt / intt / polymul of the JS host (pragma-dsp_amd/js `.ntt`, through the N-API addon) against the Python-integer
reference of tests/ntt_ref.py, on BigUint64Array, BigInt64Array and arrays of BigInt, at the vectors of the host-form
test of test_gpu_ntt (N = 64 and 4096); the error texts; and the root's key list, which `.ntt` must not join.  Equality
of 64-bit integers, no tolerance."""
import functools

import pytest

import js_host
import ntt_ref
from ntt_ref import P

pytestmark = [pytest.mark.gpu, js_host.needs_node]
run_cases = functools.partial(js_host.run_cases, "ntt_cases.js", tail=2)


def strs(v):
    return [str(x) for x in v]


def test_js_ntt_against_the_reference(tmp_path):
    cases, want = [], []
    for n in (64, 4096):
        xs = ntt_ref.rows(n, 3, 0, seed=n)  # the rows of test_gpu_ntt's host-form test
        for r, typed in enumerate(("u64", "i64", None)):
            x = xs[r]
            cases.append({"op": "ntt", "a": strs(x), "typed": typed})
            want.append(ntt_ref.transform_rows([x])[0])
            cases.append({"op": "intt", "a": strs(x), "typed": typed})
            want.append(ntt_ref.fast(x, inverse=True))
            la, lb = n // 2, n // 2 + 1
            cases.append({"op": "polymul", "a": strs(x[:la]), "b": strs(xs[0][:lb]), "typed": typed})
            want.append(ntt_ref.cyclic(x[:la], xs[0][:lb], n))
    cases.append({"op": "polymul", "a": strs([3, P - 1]), "b": strs([5]), "typed": "u64"})
    want.append([15, (P - 1) * 5 % P])
    got, keys, modulus = run_cases(cases, tmp_path)
    assert keys == ["spectrum", "spectrumBatch", "spectrumStream", "core", "fourier"] and int(modulus) == P
    for c, g, w in zip(cases, got, want):
        assert isinstance(g, dict) and "values" in g, (c["op"], len(c["a"]), g)
        assert [int(v) for v in g["values"]] == w, (c["op"], len(c["a"]), c["typed"])


def test_js_ntt_errors(tmp_path):
    cases = [
        {"op": "ntt", "a": strs([1] * 100), "typed": "u64"},
        {"op": "intt", "a": strs([1] * 32), "typed": "u64"},
        {"op": "ntt", "a": strs([1] * 32768), "typed": "u64"},
        {"op": "ntt", "a": [1.0, 2.0], "raw": True},
        {"op": "polymul", "a": strs([1] * 9000), "b": strs([1] * 8000), "typed": "u64"},
        {"op": "polymul", "a": [], "b": strs([1]), "typed": "u64"},
    ]
    got, _, _ = run_cases(cases, tmp_path)
    assert [g["error"] for g in got] == [
        "NTT size must be power of two, got 100",
        "NTT size 32 is outside 64 ... 16384",
        "NTT size 32768 is outside 64 ... 16384",
        "values must be a BigUint64Array, a BigInt64Array or an array of BigInt",
        "the product of 9000 and 8000 coefficients needs a transform of 1 ... 16384 points",
        "the product of 0 and 1 coefficients needs a transform of 1 ... 16384 points",
    ]

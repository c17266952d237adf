"""The refusals of the element-wise entry points (pdsp_complex_op_f32, pdsp_apply_window_*, pdsp_magnitude_*,
pdsp_phase_*) are all decided before anything is launched, so they are tested here without a device, through the C
ABI with made-up pointer values.  Only calls that must be refused, or that return before the launch (count == 0), are
made: a call the library accepts would launch on a made-up pointer.  The accepting side of every boundary is in
test_gpu_elementwise.py, with real buffers.

The aliasing rule (include/pdsp_hip.h): an output may share bytes with an input of the same extent only where the two
begin at the same address; out_re and out_im share nothing; a broadcast b and a window share nothing with the output.
Each rule is probed at its boundary: one byte of overlap, from either side, is refused."""
import ctypes as C

import pytest

vp = C.c_void_p

N = 1024
A_RE, A_IM, B_RE, B_IM, O_RE, O_IM = (k << 20 for k in range(1, 7))  # six planes, 1 MiB apart
OVERLAP = b"output overlaps input"
MUL, CONJ = 2, 4


@pytest.fixture(scope="module")
def lib(pdsp):
    return pdsp.lib


def _refused(lib, rc, msg=OVERLAP):
    from pragma_dsp_amd import _capi
    assert rc == _capi.ERR_BAD_ARG
    assert lib.pdsp_last_error() == msg, lib.pdsp_last_error()


def cx(lib, op=MUL, count=N, a_re=A_RE, a_im=A_IM, b_re=B_RE, b_im=B_IM, b_len=N, o_re=O_RE, o_im=O_IM):
    p = [None if v is None else vp(v) for v in (a_re, a_im, b_re, b_im)]
    return lib.pdsp_complex_op_f32(op, count, p[0], p[1], p[2], p[3], b_len, 0.0, 0.0,
                                   None if o_re is None else vp(o_re), None if o_im is None else vp(o_im), None)


def test_complex_op_out_planes_must_not_meet(lib):
    nb = 4 * N
    for o_im in (O_RE, O_RE + 4, O_RE + nb - 1, O_RE - nb + 1):
        _refused(lib, cx(lib, o_im=o_im))
        _refused(lib, cx(lib, op=CONJ, o_im=o_im, b_re=None, b_im=None, b_len=0))


@pytest.mark.parametrize("plane", ["a_re", "a_im", "b_re", "b_im"])
@pytest.mark.parametrize("out", ["o_re", "o_im"])
def test_complex_op_partial_overlap_with_a_full_length_input(lib, plane, out):
    nb = 4 * N
    base = {"o_re": O_RE, "o_im": O_IM}[out]
    # one element up or down, and one byte of overlap at either end
    for delta in (4, -4, nb - 1, -(nb - 1), 1):
        _refused(lib, cx(lib, **{plane: base + delta}))
    if plane.startswith("a"):  # the unary ops have a only
        for delta in (4, -(nb - 1)):
            _refused(lib, cx(lib, op=CONJ, b_re=None, b_im=None, b_len=0, **{plane: base + delta}))


@pytest.mark.parametrize("plane", ["b_re", "b_im"])
@pytest.mark.parametrize("out", ["o_re", "o_im"])
def test_complex_op_broadcast_b_shares_no_byte_with_out(lib, plane, out):
    nb, b_len = 4 * N, 256
    bb = 4 * b_len
    base = {"o_re": O_RE, "o_im": O_IM}[out]
    # row 0 of out (the same address is no excuse here), a later row, and one byte at either end
    for addr in (base, base + bb, base + nb - bb, base - bb + 1, base + nb - 1):
        _refused(lib, cx(lib, b_len=b_len, **{plane: addr}))
    _refused(lib, cx(lib, b_len=1, **{plane: base + nb - 4}))  # the last element of out as a one-value b


def test_complex_op_argument_errors(lib):
    from pragma_dsp_amd import _capi
    _refused(lib, cx(lib, count=-1), b"negative size")
    _refused(lib, cx(lib, count=(1 << 63) - 1), b"count 9223372036854775807 overflows")
    _refused(lib, cx(lib, count=1 << 60), b"count 1152921504606846976 overflows")
    for op in (-1, 7, 100):
        _refused(lib, cx(lib, op=op), b"unknown complex op %d" % op)
        _refused(lib, cx(lib, op=op, count=0), b"unknown complex op %d" % op)
    for name in ("a_re", "a_im", "o_re", "o_im", "b_re", "b_im"):
        _refused(lib, cx(lib, **{name: None}), b"null buffer")
    for name in ("a_re", "a_im", "o_re", "o_im"):
        _refused(lib, cx(lib, op=CONJ, b_re=None, b_im=None, b_len=0, **{name: None}), b"null buffer")
    for b_len in (0, -4, 3, 1000, 2 * N):
        _refused(lib, cx(lib, b_len=b_len), b"second operand length %d must divide %d" % (b_len, N))
    # count == 0 returns before the pointers are looked at
    for op in range(7):
        assert cx(lib, op=op, count=0, o_im=O_RE, b_len=0) == _capi.OK
        assert cx(lib, op=op, count=0, a_re=None, a_im=None, b_re=None, b_im=None, o_re=None, o_im=None) == _capi.OK


@pytest.mark.parametrize("sfx,es", [("f32", 4), ("f64", 8)])
def test_apply_window_refusals(lib, sfx, es):
    from pragma_dsp_amd import _capi
    f = getattr(lib, "pdsp_apply_window_" + sfx)
    batch, n = 8, 128
    nb, wb = batch * n * es, n * es
    IN, WIN, OUT = A_RE, B_RE, O_RE

    def call(batch=batch, n=n, i=IN, w=WIN, o=OUT):
        return f(batch, n, None if i is None else vp(i), None if w is None else vp(w), None if o is None else vp(o),
                 None)

    for delta in (es, -es, nb - 1, -(nb - 1), 1, n * es):  # partial overlap of out and in; a whole row counts
        _refused(lib, call(o=IN + delta))
    for w in (OUT, OUT + es, OUT + nb - 1, OUT - wb + 1, OUT + 3 * wb):  # window anywhere inside out
        _refused(lib, call(w=w))
    _refused(lib, call(o=IN, w=IN))  # in place is fine, but not with the window in the same bytes
    _refused(lib, call(batch=-1), b"negative size")
    _refused(lib, call(n=-1), b"negative size")
    _refused(lib, call(batch=1 << 40, n=1 << 40), b"batch 1099511627776 x n overflows")
    _refused(lib, call(batch=(1 << 63) - 1, n=2), b"batch 9223372036854775807 x n overflows")
    _refused(lib, call(batch=1 << 31, n=1 << 30), b"batch 2147483648 x n overflows")  # the byte count overflows
    for name in ("i", "w", "o"):
        _refused(lib, call(**{name: None}), b"null buffer")
    for b0, n0 in ((0, n), (batch, 0), (0, 0), (1 << 62, 0)):
        assert call(batch=b0, n=n0, o=IN + es) == _capi.OK  # nothing to do: returns before the pointers matter
        assert call(batch=b0, n=n0, i=None, w=None, o=None) == _capi.OK


@pytest.mark.parametrize("sfx,es", [("f32", 4), ("f64", 8)])
@pytest.mark.parametrize("name", ["magnitude", "phase"])
def test_polar_refusals(lib, name, sfx, es):
    from pragma_dsp_amd import _capi
    f = getattr(lib, f"pdsp_{name}_{sfx}")
    nb = N * es
    RE, IM, OUT = A_RE, A_IM, O_RE

    def call(count=N, re=RE, im=IM, o=OUT):
        return f(count, None if re is None else vp(re), None if im is None else vp(im),
                 None if o is None else vp(o), None)

    for base in (RE, IM):
        for delta in (es, -es, nb - 1, -(nb - 1), 1):
            _refused(lib, call(o=base + delta))
    _refused(lib, call(re=OUT, im=OUT + es))  # out == re is fine, im one element further is not
    _refused(lib, call(count=-1), b"negative size")
    _refused(lib, call(count=1 << 60), b"count 1152921504606846976 overflows")
    for arg in ("re", "im", "o"):
        _refused(lib, call(**{arg: None}), b"null buffer")
    assert call(count=0, o=RE + es) == _capi.OK
    assert call(count=0, re=None, im=None, o=None) == _capi.OK


def test_vec4_query_names_every_condition(lib):
    """pdsp_dev_complex_op_vec4 is the predicate launch_complex_op itself calls: each of its conditions alone turns
    the 16-byte path off, and a condition that does not apply to a unary op is not looked at."""
    from pragma_dsp_amd import _capi

    def q(op=MUL, count=N, a_re=A_RE, a_im=A_IM, b_re=B_RE, b_im=B_IM, b_len=N, o_re=O_RE, o_im=O_IM):
        got = C.c_int(-1)
        assert lib.pdsp_dev_complex_op_vec4(op, count, vp(a_re), vp(a_im), vp(b_re), vp(b_im), b_len, vp(o_re),
                                            vp(o_im), C.byref(got)) == _capi.OK
        return got.value

    for op in range(7):
        binary = op <= 3
        assert q(op=op) == 1
        for name, base in (("a_re", A_RE), ("a_im", A_IM), ("o_re", O_RE), ("o_im", O_IM)):
            for off in (4, 8, 12):
                assert q(op=op, **{name: base + off}) == 0, (op, name, off)
            assert q(op=op, **{name: base + 16}) == 1
        for name, base in (("b_re", B_RE), ("b_im", B_IM)):
            for off in (4, 8, 12):
                assert q(op=op, **{name: base + off}) == (0 if binary else 1), (op, name, off)
        for r in (1, 2, 3):
            assert q(op=op, count=N + r, b_len=N + r) == 0
            assert q(op=op, count=6 * 512, b_len=4 + r) == (0 if binary else 1)
        assert q(op=op, count=0, b_len=0) == 1 and q(op=op, b_len=4) == 1 and q(op=op, b_len=1) == (0 if binary else 1)
    _refused(lib, lib.pdsp_dev_complex_op_vec4(7, N, vp(A_RE), vp(A_IM), None, None, 0, vp(O_RE), vp(O_IM),
                                               C.byref(C.c_int())), b"unknown complex op 7")
    _refused(lib, lib.pdsp_dev_complex_op_vec4(0, N, vp(A_RE), vp(A_IM), None, None, 0, vp(O_RE), vp(O_IM), None),
             b"null buffer")


def test_header_states_the_rule(pdsp):
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"\s*\n \*\s*", " ", open(os.path.join(root, "include", "pdsp_hip.h")).read())
    for phrase in ("only where the two begin at the same address", "out_re and out_im must not overlap each other",
                   "a broadcast b must share no byte with either out plane", "\"output overlaps input\"",
                   "overlapping window, is refused"):
        assert phrase in header, phrase

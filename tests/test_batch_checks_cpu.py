"""The element-wise device helpers of batch.py hand raw pointers to the library: an operand that is not a CUDA
tensor must be refused in Python, before any library call.  The library is replaced by a recorder, so a missing
check shows up as a recorded call instead of a kernel launch on a host pointer."""
import numpy as np
import pytest


class Recorder:
    """Stands in for the ctypes library: every function called on it is recorded and returns 0 (PDSP_OK)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append(name)
            return 0
        return fn


@pytest.fixture
def recorder(pdsp, monkeypatch):
    from pragma_dsp_amd import batch
    rec = Recorder()
    monkeypatch.setattr(batch, "lib", rec)
    return rec


def _host_cases():
    import torch
    from pragma_dsp_amd import batch as B
    a = torch.ones((2, 8))
    a64 = torch.ones((2, 8), dtype=torch.float64)
    w = torch.ones(8)
    return [
        ("magnitude", lambda: B.magnitude(a, a)),
        ("magnitude_f64", lambda: B.magnitude(a64, a64)),
        ("phase", lambda: B.phase(a, a)),
        ("apply_window", lambda: B.apply_window(a, w)),
        ("complex_mul", lambda: B.complex_mul((a, a), (a, a))),
        ("complex_conj", lambda: B.complex_conj((a, a))),
        ("complex_scale", lambda: B.complex_scale((a64, a64), 2.0)),
        ("complex_div_scalar", lambda: B.complex_div_scalar((a, a), 1.0, 2.0)),
    ]


def test_host_operands_are_refused_before_any_library_call(pdsp, recorder):
    from pragma_dsp_amd._capi import ERR_BAD_ARG
    for name, call in _host_cases():
        with pytest.raises(pdsp.PdspError) as e:
            call()
        assert e.value.code == ERR_BAD_ARG, name
    assert recorder.calls == []


def test_numpy_operands_are_refused(pdsp, recorder):
    from pragma_dsp_amd import batch as B
    x = np.ones(8, dtype=np.float32)
    with pytest.raises(pdsp.PdspError):
        B.magnitude(x, x)
    with pytest.raises(pdsp.PdspError):
        B.complex_add((x, x), (x, x))
    assert recorder.calls == []

"""The Hilbert kernels' resources in the built library: the design of pdsp_hilbert_kernel.h rests on the row's samples
being loaded a second time instead of staying in registers across the transforms, which empty asm statements keep the
compiler from undoing.  A silent merge would not spill; it would cost workgroups per CU.  So every FAST instantiation
must keep the occupancy of fir_overlap_save_kernel's FAST instantiation at the same N and precision (the issue's
condition), every general one must not fall below the rows recorded in DESIGN.md 4.8, and none may use scratch."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIB = os.path.join(ROOT, "pragma-dsp_amd", "csrc", "libpdsp_hip.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="needs the built library and the LLVM tools")


@pytest.fixture(scope="module")
def table():
    import kernel_resources
    return {r["kernel"]: r for r in kernel_resources.kernels(LIB)}


def test_all_thirty_six_kernels_are_built_without_scratch(table):
    rows = [r for k, r in table.items() if k.startswith("hilbert_kernel<")]
    assert len(rows) == 36
    for r in rows:
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0, r["kernel"]


@pytest.mark.parametrize("t", ["float", "double"])
@pytest.mark.parametrize("log2m", range(5, 14))
def test_fast_path_keeps_the_fir_kernels_occupancy(table, t, log2m):
    h = table[f"hilbert_kernel<{t}, {log2m}, true>"]
    f = table[f"fir_overlap_save_kernel<{t}, {log2m}, true>"]
    assert h["group_segment_fixed_size"] == f["group_segment_fixed_size"]
    assert h["workgroups_per_cu"] == f["workgroups_per_cu"] == {"float": 4, "double": 2}[t] // (2 if log2m == 13 else 1)


@pytest.mark.parametrize("t", ["float", "double"])
@pytest.mark.parametrize("log2m", range(5, 14))
def test_general_path_keeps_its_recorded_occupancy(table, t, log2m):
    h = table[f"hilbert_kernel<{t}, {log2m}, false>"]
    if t == "double":
        want = 1 if log2m == 13 else 2
    else:
        want = 4 if log2m <= 8 else (1 if log2m == 13 else 3)  # the recorded miss against FIR's 4 / 2
    assert h["workgroups_per_cu"] >= want, (h["vgpr_count"], h["workgroups_per_cu"])

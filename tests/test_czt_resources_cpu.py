"""The chirp-z transform kernels' resources in the built library: all eighteen czt_kernel instantiations (f32 / f64 x
M = 32 ... 8192) exist, none uses scratch or spills, and each holds the LDS of bluestein_kernel at the same M and
precision (one padded complex row of M points per transform: the two kernels run the same pass sets).  The epilogue's
table is loaded behind both transforms instead of being held across them; a silent hoist would cost registers, not
spill, so the VGPR counts and workgroups per CU are printed here and recorded in DESIGN.md 4.13 rather than asserted
against a wished-for value."""
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


def test_all_eighteen_kernels_are_built_without_scratch(table):
    rows = {k: r for k, r in table.items() if k.startswith("czt_kernel<")}
    assert set(rows) == {f"czt_kernel<{t}, {l}>" for t in ("float", "double") for l in range(5, 14)}
    for k, r in rows.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, k


@pytest.mark.parametrize("t", ["float", "double"])
@pytest.mark.parametrize("log2m", range(5, 14))
def test_lds_is_the_any_length_dfts(table, t, log2m):
    c = table[f"czt_kernel<{t}, {log2m}>"]
    b = table[f"bluestein_kernel<{t}, {log2m}>"]
    assert c["group_segment_fixed_size"] == b["group_segment_fixed_size"]
    print(f"CZTRES {t} log2m={log2m} vgprs={c['vgpr_count']} wg/cu={c['workgroups_per_cu']} "
          f"(bluestein_kernel: {b['vgpr_count']}, {b['workgroups_per_cu']})")

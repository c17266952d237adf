"""The NTT kernels' resources in the built library: every instantiation the dispatch can reach exists -- forward (0),
inverse (1) and CONV (2) at each of 2^6 ... 2^14 points, and the element-wise product -- none spills or uses scratch,
and DESIGN.md 4.14's table names the same kernels.  Their LDS is dynamic (no static bytes): N + N / 16 values of 8
bytes per row, which the table records per launch.  VGPRs and workgroups per CU are printed and recorded in DESIGN.md
4.14, not asserted against a wished-for value -- but CONV at N = 16384 runs 1024 threads and so must fit 128 VGPRs."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIB = os.path.join(ROOT, "pragma-dsp_amd", "csrc", "libpdsp_hip.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="needs the built library and the LLVM tools")

NAMES = {f"ntt_kernel<{l}, {op}>" for l in range(6, 15) for op in (0, 1, 2)} | {"ntt_mul_kernel"}


def threads(name):
    """Workgroup size of an instantiation (pdsp_ntt_kernel.h, NttTraits): N / E threads per row, a wave at least."""
    if name == "ntt_mul_kernel":
        return 256
    l, op = (int(v) for v in re.findall(r"\d+", name))
    e = 16 if op == 2 or l >= 11 else 8
    return max(64, (1 << l) // e)


@pytest.fixture(scope="module")
def table():
    import kernel_resources
    return {r["kernel"]: r for r in kernel_resources.kernels(LIB) if r["kernel"].startswith("ntt_")}


def test_every_instantiation_is_built_without_scratch_or_static_lds(table):
    assert set(table) == NAMES
    for k, r in sorted(table.items()):
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, k
        assert r["group_segment_fixed_size"] == 0 and r["max_flat_workgroup_size"] == threads(k), k
        print(f"NTTRES {k} vgprs={r['vgpr_count']} sgprs={r['sgpr_count']} wg/cu by registers={r['workgroups_per_cu']}")
    assert table["ntt_kernel<14, 2>"]["vgpr_count"] <= 128 and table["ntt_kernel<14, 0>"]["vgpr_count"] <= 128


def test_the_recorded_table_lists_the_same_kernels():
    """`| ntt_kernel<...> | vgprs | ... |` rows of DESIGN.md 4.14"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.14"):]
    sec = sec[:sec.index("\n## ")] if "\n## " in sec else sec
    rows = set(re.findall(r"^\| `(ntt_\w*kernel(?:<[^`]+>)?)` \|", sec, re.M))
    assert rows == NAMES

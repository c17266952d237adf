"""The sliding DFT kernels' resources in the built library: every instantiation the dispatch can reach exists --
sdft_kernel<float, 4> (N <= 1024), <float, 8> (N > 1024) and <double, 4> (every N; pdsp_internal.h, sdft_segment) --
none spills or uses scratch, each runs 256 threads on the static LDS of its exchange words and round totals, and
DESIGN.md 4.15's table names the same kernels.  VGPRs and workgroups per CU are printed and recorded there, not
asserted against a wished-for value."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIB = os.path.join(ROOT, "pragma-dsp_amd", "csrc", "libpdsp_hip.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="needs the built library and the LLVM tools")

NAMES = {"sdft_kernel<float, 4>", "sdft_kernel<float, 8>", "sdft_kernel<double, 4>"}


@pytest.fixture(scope="module")
def table():
    import kernel_resources
    return {r["kernel"]: r for r in kernel_resources.kernels(LIB) if r["kernel"].startswith("sdft_")}


def test_every_instantiation_is_built_without_spills_or_scratch(table):
    assert set(table) == NAMES
    for k, r in sorted(table.items()):
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, k
        # [2][2][4 waves] exchange words + [2][5 components][16 rounds] totals, complex
        elem = 16 if "double" in k else 8
        assert r["group_segment_fixed_size"] == (2 * 2 * 4 + 2 * 5 * 16) * elem, k
        assert r["max_flat_workgroup_size"] == 256, k
        print(f"SDFTRES {k} vgprs={r['vgpr_count']} sgprs={r['sgpr_count']} lds={r['group_segment_fixed_size']} "
              f"wg/cu by registers={r['workgroups_per_cu']}")


def test_the_dispatch_rule_reaches_exactly_these():
    """sdft_segment (pdsp_internal.h) and the launch (pdsp_kernels_sdft.hip) name E = 4 and 8 for f32, 4 for f64."""
    src = open(os.path.join(ROOT, "pragma-dsp_amd", "csrc", "pdsp_internal.h")).read()
    assert "inline int sdft_segment(long long n, size_t elem) { return elem == 4 && n > 1024 ? 8 : 4; }" in src
    unit = open(os.path.join(ROOT, "pragma-dsp_amd", "csrc", "pdsp_kernels_sdft.hip")).read()
    assert sorted(re.findall(r"go\(int_c<(\d+)>\{\}\)", unit)) == ["4", "4", "8"]
    import sdft_ref
    for n in (2, 1024, 1025, 16384):
        assert sdft_ref.segment(n, "f32") == (8 if n > 1024 else 4) and sdft_ref.segment(n, "f64") == 4


def test_the_recorded_table_lists_the_same_kernels():
    """`| sdft_kernel<...> | vgprs | ... |` rows of DESIGN.md 4.15"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.15"):]
    sec = sec[:sec.index("\n## ")] if "\n## " in sec else sec
    rows = set(re.findall(r"^\| `(sdft_kernel<[^`]+>)` \|", sec, re.M))
    assert rows == NAMES

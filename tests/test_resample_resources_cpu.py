"""The rate-change kernels' resources in the built library against what DESIGN.md 4.9 records: the number of
upfirdn_kernel instantiations, none with scratch or a spilled register, and each at no fewer workgroups per CU (by
registers: LDS is dynamic, sized per launch by the tile rule) than its row of the table there."""
import os
import re
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
    return {r["kernel"]: r for r in kernel_resources.kernels(LIB) if r["kernel"].startswith("upfirdn_kernel<")}


@pytest.fixture(scope="module")
def recorded():
    """`| upfirdn_kernel<...> | vgprs | workgroups per CU |` rows of DESIGN.md 4.9, and its stated count."""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.9"):]
    sec = sec[:sec.index("\n## ")] if "\n## " in sec else sec
    rows = {m.group(1): int(m.group(2))
            for m in re.finditer(r"^\| `(upfirdn_kernel<[^`]+>)` \|[^|]*\| *(\d+) *\|", sec, re.M)}
    count = int(re.search(r"(\d+) instantiations of `upfirdn_kernel`", sec).group(1))
    return rows, count


def test_no_instantiation_uses_scratch_or_spills(table):
    assert table
    for name, r in table.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, name


def test_the_instantiations_are_the_ones_design_md_lists(table, recorded):
    rows, count = recorded
    assert len(table) == count == len(rows)
    assert set(table) == set(rows)


def test_each_instantiation_keeps_its_recorded_occupancy(table, recorded):
    rows, _ = recorded
    for name, want in rows.items():
        assert table[name]["workgroups_per_cu"] >= want, (name, table[name]["vgpr_count"])

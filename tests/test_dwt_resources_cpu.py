"""The wavelet kernels' resources in the built library: all eight instantiations (forward / inverse x f32 / f64 x
resident / tiled) exist, and none uses scratch or spills.  Their LDS is dynamic -- no static bytes -- and sized per
launch by the tile rule, whose formulas DESIGN.md 4.12 states; this file holds the rule to those formulas.  VGPRs and
workgroups per CU are printed and recorded in DESIGN.md 4.12, not asserted against a wished-for value."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIB = os.path.join(ROOT, "pragma-dsp_amd", "csrc", "libpdsp_hip.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="needs the built library and the LLVM tools")

NAMES = {f"dwt_{d}_kernel<{t}, {r}>" for d in ("forward", "inverse") for t in ("float", "double")
         for r in ("true", "false")}


@pytest.fixture(scope="module")
def table():
    import kernel_resources
    return {r["kernel"]: r for r in kernel_resources.kernels(LIB) if r["kernel"].startswith("dwt_")}


def test_all_eight_kernels_are_built_without_scratch_or_static_lds(table):
    assert set(table) == NAMES
    for k, r in sorted(table.items()):
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, k
        assert r["group_segment_fixed_size"] == 0 and r["max_flat_workgroup_size"] == 256, k
        print(f"DWTRES {k} vgprs={r['vgpr_count']} sgprs={r['sgpr_count']} wg/cu by registers={r['workgroups_per_cu']}")


def test_the_recorded_table_lists_the_same_kernels(table):
    """`| dwt_..._kernel<...> | vgprs | ... |` rows of DESIGN.md 4.12"""
    import re
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = text[text.index("### 4.12"):]
    sec = sec[:sec.index("\n## ")] if "\n## " in sec else sec
    rows = set(re.findall(r"^\| `(dwt_\w+_kernel<[^`]+>)` \|", sec, re.M))
    assert rows == NAMES


@pytest.mark.parametrize("eb", [4, 8])
def test_dynamic_lds_is_what_design_md_states(pdsp, eb):
    prev = pdsp.lib.pdsp_set_dwt_tile(0)
    try:
        for f, levels, n in ((2, 1, 2), (8, 6, 4096), (20, 12, 4096), (8, 4, 1 << 16), (16, 8, 1 << 20), (32, 5, 3 << 16)):
            g = f - 2
            for inverse in (0, 1):
                info = (C.c_longlong * 5)()
                assert pdsp.lib.pdsp_dev_dwt_tile(f, levels, n, eb, inverse, info) == 0
                resident, t, halo, lds, tiles = info
                if resident:
                    want = n + n // 2 + (n // 4 if inverse else 0)
                elif inverse:
                    want = (t // 2 + g) + (t // 2 + g) + (t // 4 + g)
                else:
                    assert halo == g * ((1 << levels) - 1)
                    want = (t + halo) + (t + halo - g) // 2
                assert lds == want * eb <= 163840, (f, levels, n, inverse)
    finally:
        pdsp.lib.pdsp_set_dwt_tile(prev)

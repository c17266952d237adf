"""The 2-D transform's kernels in the built library (tools/kernel_resources.py): every instantiation the decision
function can reach exists, none uses scratch or spills, the resident kernels hold exactly the LDS of the 4096-point row
kernel -- (4096 + 256) complex values, the one-pad-per-16 layout -- and the workgroups per CU are the ones DESIGN.md
4.18 records: the design target (4 in f32 as fft_stockham_kernel<float, 12>, 2 in f64) on every resident shape, and the
column kernels as compiled."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIB = os.path.join(ROOT, "pragma-dsp_amd", "csrc", "libpdsp_hip.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                                reason="needs the built library and the LLVM tools")

RESIDENT = [(a, b) for a in range(4, 9) for b in range(4, 9) if a + b <= 12]
# (log2 H, tile) of the column tile kernel by precision: the tiles of the decision function
TILES = {"float": [(6, 64), (7, 32), (8, 32), (9, 16), (9, 32)], "double": [(6, 64), (7, 32), (8, 16), (9, 16)]}
# workgroups per CU as compiled
TILE_WG = {("float", 6, 64): 4, ("float", 7, 32): 4, ("float", 8, 32): 2, ("float", 9, 16): 2, ("float", 9, 32): 1,
           ("double", 6, 64): 2, ("double", 7, 32): 2, ("double", 8, 16): 2, ("double", 9, 16): 1}
# the register column kernels hold no LDS: registers alone bound them.  (workgroups per CU as compiled, the VGPR count
# that keeps them: 512 / 128 = 4 waves per SIMD, 512 / 256 = 2, 512 / 168 = 3, 512 / 512 = 1)
REG_WG = {("float", 4): (4, 128), ("float", 5): (2, 256), ("double", 4): (3, 168), ("double", 5): (1, 512)}


@pytest.fixture(scope="module")
def table():
    import kernel_resources
    return {r["kernel"]: r for r in kernel_resources.kernels(LIB)}


def test_every_kernel_is_built_without_scratch(table):
    rows = {k: r for k, r in table.items() if k.startswith("fft2d_")}
    want = {f"fft2d_resident_kernel<{t}, {a}, {b}>" for t in ("float", "double") for a, b in RESIDENT}
    want |= {f"fft2d_cols_tile_kernel<{t}, {lh}, {tile}>" for t, v in TILES.items() for lh, tile in v}
    want |= {f"fft2d_cols_reg_kernel<{t}, {lh}>" for t in ("float", "double") for lh in (4, 5)}
    assert set(rows) == want
    for k, r in rows.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, k


@pytest.mark.parametrize("t,elem", [("float", 8), ("double", 16)])
@pytest.mark.parametrize("lh,lw", RESIDENT)
def test_resident_kernels_hold_the_row_kernels_lds_and_occupancy(table, t, elem, lh, lw):
    r = table[f"fft2d_resident_kernel<{t}, {lh}, {lw}>"]
    row = next(v for k, v in table.items()
               if k.startswith(f"fft_stockham_kernel<{t}, 12, LoadComplex<{t}>, StoreComplex<{t}>"))
    assert r["group_segment_fixed_size"] == (4096 + 256) * elem == row["group_segment_fixed_size"]
    target = 4 if t == "float" else 2
    assert row["workgroups_per_cu"] == target
    print(f"FFT2RES {t} {1 << lh}x{1 << lw} vgprs={r['vgpr_count']} wg/cu={r['workgroups_per_cu']}")
    assert r["workgroups_per_cu"] == target and r["vgpr_count"] <= (128 if t == "float" else 256)


@pytest.mark.parametrize("key", sorted(TILE_WG), ids=lambda k: f"{k[0]}-{k[1]}-{k[2]}")
def test_column_tile_kernels_as_compiled(table, key):
    t, lh, tile = key
    r = table[f"fft2d_cols_tile_kernel<{t}, {lh}, {tile}>"]
    n = 1 << lh
    lrow = n + n // 16
    pitch = lrow + (2 - lrow % 8) % 8  # tile_pass_kernel's LROWX
    assert r["group_segment_fixed_size"] == tile * pitch * (8 if t == "float" else 16)
    print(f"FFT2RES tile {t} H={n} tile={tile} vgprs={r['vgpr_count']} wg/cu={r['workgroups_per_cu']}")
    assert r["workgroups_per_cu"] == TILE_WG[key]


@pytest.mark.parametrize("key", sorted(REG_WG), ids=lambda k: f"{k[0]}-{k[1]}")
def test_column_register_kernels_as_compiled(table, key):
    t, lh = key
    r = table[f"fft2d_cols_reg_kernel<{t}, {lh}>"]
    wg, vgprs = REG_WG[key]
    print(f"FFT2RES reg {t} H={1 << lh} vgprs={r['vgpr_count']} wg/cu={r['workgroups_per_cu']}")
    assert r["group_segment_fixed_size"] == 0
    assert r["workgroups_per_cu"] == wg and r["vgpr_count"] <= vgprs

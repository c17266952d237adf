"""The case table and the batch arithmetic of tests/test_gpu_full_machine.py (tests/full_machine_cases.py), without a
GPU: every case fills the machine by the restated launch formulas, ends in a partial workgroup where a workgroup holds
several rows, stays under 12 GiB, the byte-line cases cross their lines, the f64 ISTFT case makes four chunks, the
periodic signal is periodic bit for bit, and the comparator names the position it is given."""
import math

import numpy as np
import pytest

import full_machine_cases as FM

CUS = [256, 104]  # the MI355X, and another count (no power of two)
ALL = FM.PLAIN + FM.LINES + FM.VARIANTS


def test_the_table_names_every_family_and_no_case_twice():
    assert len(set(ALL)) == len(ALL)
    assert {c.family for c in FM.PLAIN} == {"dct", "hilbert", "fir", "stft", "istft", "dft", "czt", "dwt", "upfirdn",
                                            "sdft", "ntt"}
    assert {c.family for c in FM.LINES} == {"dct", "fir", "dwt", "upfirdn"} and all(c.line for c in FM.LINES)
    assert {c.variant for c in FM.VARIANTS} == {"inplace", "fast", "odd"}
    assert len({FM.case_id(c) for c in ALL}) == len(ALL)


@pytest.mark.parametrize("cus", CUS)
def test_every_case_fills_the_machine_and_ends_in_a_partial_workgroup(cus):
    for c in ALL:
        g = FM.geometry(c)
        b = FM.rows_of(c, cus)
        assert FM.workgroups(c, b) >= FM.ROUNDS * cus, FM.case_id(c)
        assert b > FM.K, FM.case_id(c)  # one whole group and a remainder at least
        assert g.r & (g.r - 1) == 0 and math.gcd(FM.K, g.r) == 1, FM.case_id(c)
        if g.r > 1:
            assert (b * g.per_row) % g.r != 0, FM.case_id(c)
            assert math.gcd(FM.K * g.per_row, g.r) == 1, FM.case_id(c)  # every base row visits every slot
        assert FM.live_bytes(c, b) <= FM.LIVE_LIMIT, (FM.case_id(c), FM.live_bytes(c, b))
        for v in (g.vin, g.vout):
            stride = FM.stride_of(c, v)
            if c.variant == "fast":
                assert v < stride <= v + 16 // FM.ELEM[c.dt] and (stride * FM.ELEM[c.dt]) % 16 == 0
            elif c.variant == "odd":
                assert v < stride <= v + 3 and stride % 2 == 1
            else:
                assert stride == v


def test_rows_per_workgroup_are_the_families_own():
    import ntt_model
    assert [FM.packed_rows(n // 2) for n in FM.PACKED_NS] == [128, 4, 1]
    assert [FM.packed_rows(FM.conv_size(2 * ln - 1)) for ln in FM.DFT_LS] == [128, 2, 1]
    assert [FM.conv_size(ln + k - 1) for ln, k in FM.CZT_SHAPES] == [32, 2048, 8192]
    ops = {"forward": ntt_model.FORWARD, "inverse": ntt_model.INVERSE, "convolve": ntt_model.CONV}
    for lg in range(6, 15):
        for name, op in ops.items():
            assert FM.ntt_rows(lg, name) == ntt_model.rows_per_workgroup(lg, op)
    for n in FM.PACKED_NS:
        ntaps, length = FM.fir_shape(n)
        assert ntaps % 2 == 1 and 2 * ntaps <= n and FM.fir_blocks(n, ntaps, length) == 3 and length % 2 == 0


def test_dwt_cases_are_resident_and_tiled_as_named():
    for c in FM.PLAIN:
        if c.family == "dwt":
            n, levels, key = c.shape
            resident, tiles = FM.dwt_tiles(FM.DWT_TAPS[key], levels, n, c.dt, c.op == "inverse")
            assert resident == (n <= 4096) and (tiles == 1) == bool(resident), FM.case_id(c)


@pytest.mark.parametrize("cus", CUS)
def test_byte_line_cases_cross_their_lines(cus):
    for c in FM.LINES:
        b = FM.rows_of(c, cus)
        assert b == FM.rows_of(c._replace(dt="f64" if c.dt == "f32" else "f32"), cus)  # one B for both precisions
        bin_, bout = FM.bytes_in_out(c, b)
        assert min(bin_, bout) > FM.LINE[c.dt], FM.case_id(c)
        g = FM.geometry(c)
        es = FM.ELEM[c.dt]
        # a whole group lies on either side of the line, and one straddles it
        assert (b - FM.K) * min(g.vin, g.vout) * es >= FM.LINE[c.dt]
    c = FM.Case("dct", 2, "f64", (16384,), None, True)
    assert FM.rows_of(c, 256) == 32768 + 61


@pytest.mark.parametrize("cus", CUS)
def test_the_f64_istft_case_makes_four_chunks_of_256_mib(cus):
    c = FM.Case("istft", None, "f64", (16384, 4096), None, False)
    assert c in FM.PLAIN
    b = FM.rows_of(c, cus)
    sf = FM.istft_chunk_frames(16384, 4096, b, 8)
    assert sf == (1 << 28) // (16384 * 8) - 3 == 2045
    assert FM.istft_chunks(16384, 4096, b, 8) >= 4
    assert FM.istft_scratch(16384, 4096, b, 8) == 1 << 28
    assert FM.istft_chunks(2048, 2048, b, 8) == 1 and FM.istft_scratch(2048, 2048, b, 8) == 0


@pytest.mark.parametrize("n,hop", [(64, 16), (2048, 512), (2048, 2048), (16384, 4096)])
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_periodic_signal_repeats_every_61_frames_bit_for_bit(n, hop, dt):
    base = np.random.default_rng(n + hop).standard_normal((FM.K, hop)).astype(dt)
    frames = 3 * FM.K + 7
    x = FM.periodic_signal(base, frames, n)
    assert x.dtype == dt and x.size == (frames - 1) * hop + n
    it = np.int32 if dt == np.float32 else np.int64
    fr = x[np.arange(frames)[:, None] * hop + np.arange(n)[None, :]].view(it)
    assert np.array_equal(fr[FM.K:], fr[:-FM.K])
    assert not np.array_equal(fr[1:FM.K], fr[:FM.K - 1])  # and no shorter period by chance


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_the_comparator_names_the_flipped_bits(dt):
    import torch
    it = torch.int32 if dt == "f32" else torch.int64
    cols, groups, rem = 37, 9, 23
    b = groups * FM.K + rem
    ref = torch.from_numpy(np.random.default_rng(3).integers(-2 ** 31, 2 ** 31, (FM.K, cols))).to(it)
    out = ref[torch.arange(b) % FM.K].clone()
    c = FM.Case("dct", 2, dt, (64,), None, False)  # 128 rows per workgroup
    for slice_elems in (FM.SLICE, 2 * FM.K * cols, 1):  # one slice, slices of two groups, of one
        assert FM.first_mismatch(out, ref, slice_elems) is None
    a = ((groups - 1) * FM.K + 40, 11)   # in the last whole group
    z = (groups * FM.K + rem - 1, cols - 1)  # in the remainder: the last element of all
    out[a] ^= 1 << 20
    out[z] ^= 1
    for slice_elems in (FM.SLICE, 2 * FM.K * cols, 1):
        row, col, got, want = FM.first_mismatch(out, ref, slice_elems)
        assert (row, col) == a and got == want ^ (1 << 20) and want == int(ref[40, 11])
    assert FM.locate(c, a[0]) == (a[0] // 128, a[0] % 128)
    text = FM.describe(c, row, col, got, want)
    assert f"row {a[0]} (base row 40), workgroup {a[0] // 128}, slot {a[0] % 128}, column 11" in text
    out[a] ^= 1 << 20
    row, col, got, want = FM.first_mismatch(out, ref, 2 * FM.K * cols)
    assert (row, col) == z and row % FM.K == rem - 1 and got == want ^ 1
    # rows at a stride, as the padded variants hand them over
    buf = torch.zeros((b, cols + 3), dtype=it)
    buf[:, :cols] = out
    assert FM.first_mismatch(buf[:, :cols], ref, 2 * FM.K * cols)[:2] == z
    # a FIR row is three work items: the workgroup and slot are those of its first
    fir = FM.Case("fir", None, dt, (64,), None, False)
    assert FM.locate(fir, 100) == (300 // 128, 300 % 128)

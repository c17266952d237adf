"""The cases of tests/test_gpu_full_machine.py and their batch arithmetic: no GPU, no torch at import.

Every family that came after the FFT, spectrum and FIR kernels promises that a row's output depends on the row alone.
The GPU module tiles K = 61 base rows to a batch of B rows whose launch has at least W = ROUNDS x CUs workgroups and
compares every group of 61 output rows with the 61-row call, bit for bit.  ROUNDS = 32 because a CU holds at most 32
waves, which is 8 workgroups of 256 threads: W workgroups are at least four complete rounds of workgroups replacing each
other on every CU at any occupancy.  That is a condition on the launch, not a measurement.

61 is prime and every rows-per-workgroup count here is a power of two, so over the batch every base row visits every
slot of a workgroup.  Where a workgroup holds R > 1 work items, the launch has W R + R / 2 + 1 of them: its last
workgroup is partial.

Rows per workgroup, restated from the launch code (pdsp_internal.h: packed_grid; pdsp_kernels_*.hip):
  packed-real families   R = max(M / 16, 256) / (M / 16); M = N / 2 for DCT, Hilbert, STFT, the ISTFT's frames and FIR
                         (FIR's work items are rows x blocks), M = conv_size for Dft and Czt
  NTT                    NttTraits<LOG2N, OP>::ROWS (tests/ntt_model.py: rows_per_workgroup)
  DWT, upfirdn           one workgroup per tile, tiles per row from pdsp_dev_dwt_tile / pdsp_dev_upfirdn_tile
  SDFT                   ceil(chunks / tile_chunks) x bins workgroups per row
The two-pass ISTFT launches its frames chunk by chunk (pdsp_kernels_stft.hip: istft_chunk_frames, restated below); its
workgroups are counted over the chunks of one call, which run back to back on one stream."""
from collections import namedtuple

K = 61
ROUNDS = 32
LIVE_LIMIT = 12 << 30
SLICE = 1 << 28          # elements per compared slice: no temporary of the comparison exceeds 256 MiB
LINE = {"f64": 1 << 32, "f32": 1 << 31}
ELEM = {"f32": 4, "f64": 8, "u64": 8}
DTS = ("f32", "f64")

Case = namedtuple("Case", "family op dt shape variant line")
# r: work items per workgroup; per_row: work items per row; vin / vout: values per row and plane; pin / pout: planes;
# extra: scratch bytes of the call
Geometry = namedtuple("Geometry", "r per_row vin pin vout pout extra")


def case_id(c):
    shape = "x".join(str(v) for v in c.shape)
    return "-".join(str(v) for v in (c.family, c.op, shape, c.dt, c.variant) if v is not None) + ("-line" if c.line else "")


def packed_rows(m):
    tp = m // 16
    return max(tp, 256) // tp


def conv_size(total):
    """The chirp-z rows' M: the power of two >= L + K - 1, at least 32 (tests/test_dft_cpu.py, test_czt_cpu.py)."""
    return max(32, 1 << (total - 1).bit_length())


def fir_shape(n):
    """(taps, row length) of the FIR case of block N: N / 2 - 1 taps (odd: hop = N / 2 + 2), rows three blocks long."""
    return n // 2 - 1, 3 * (n // 2 + 2)


def fir_blocks(n, ntaps, y_len):
    p = ntaps if ntaps % 2 else ntaps + 1
    hop = n - (p - 1)
    return -(-y_len // hop)


def ntt_rows(log2n, op):
    log2e = 4 if op == "convolve" or log2n >= 11 else 3
    tp = (1 << log2n) >> log2e
    return 1 if tp >= 64 else 64 // tp


def sdft_segment(n, dt):
    return 8 if dt == "f32" and n > 1024 else 4


def sdft_blocks_per_row(n, t, nbins, dt):
    chunks = (t - n) // n + 1
    tc = 8 if n > 256 * sdft_segment(n, dt) else 16
    return -(-chunks // tc) * nbins


def istft_chunk_frames(n, hop, frames, elem):
    """pdsp_kernels_stft.hip, istft_chunk_frames with the development switch unset."""
    k = -(-n // hop) - 1
    sf = max((1 << 28) // (n * elem) - k, k + 1)
    sf = min(sf, (0x7fffffff - 2 * n) // hop)
    return min(sf, frames)


def istft_chunks(n, hop, frames, elem):
    return 1 if hop >= n else -(-frames // istft_chunk_frames(n, hop, frames, elem))


def istft_scratch(n, hop, frames, elem):
    if hop >= n:
        return 0
    k = -(-n // hop) - 1
    return min(istft_chunk_frames(n, hop, frames, elem) + k, frames) * n * elem


def dwt_tiles(ntaps, levels, n, dt, inverse):
    import ctypes as C

    from pragma_dsp_amd._capi import lib
    info = (C.c_longlong * 5)()
    assert lib.pdsp_dev_dwt_tile(ntaps, levels, n, ELEM[dt], int(inverse), info) == 0
    return int(info[0]), int(info[4])  # resident, tiles


def upfirdn_tiles(up, down, ntaps, y_len, dt):
    import ctypes as C

    from pragma_dsp_amd._capi import lib
    info = (C.c_longlong * 9)()
    assert lib.pdsp_dev_upfirdn_tile(up, down, ntaps, y_len, ELEM[dt], info) == 0
    return -(-y_len // (up * int(info[5])))


def upfirdn_output_len(n, up, down, ntaps):
    return ((n - 1) * up + ntaps - 1) // down + 1


DWT_TAPS = {"db2": 4, "db4": 8, "db8": 16}
SDFT_BINS = 4  # sdft_ref.path_bins


def geometry(c, frames=None):
    """The launch of a case.  frames: the batch, for the one family whose scratch depends on it (ISTFT)."""
    f, s, es = c.family, c.shape, ELEM[c.dt]
    if f == "dct":
        return Geometry(packed_rows(s[0] // 2), 1, s[0], 1, s[0], 1, 0)
    if f == "hilbert":
        return Geometry(packed_rows(s[0] // 2), 1, s[0], 1, s[0] * (2 if c.op == "analytic" else 1), 1, 0)
    if f == "fir":
        ntaps, length = fir_shape(s[0])
        return Geometry(packed_rows(s[0] // 2), fir_blocks(s[0], ntaps, length), length, 1, length, 1, 0)
    if f == "stft":  # a row is a frame; the signal holds one hop per frame
        return Geometry(packed_rows(s[0] // 2), 1, s[1], 1, s[0] // 2 + 1, 2, 0)
    if f == "istft":
        extra = istft_scratch(s[0], s[1], frames, es) if frames else 0
        return Geometry(packed_rows(s[0] // 2), 1, s[0] // 2 + 1, 2, s[1], 1, extra)
    if f == "dft":
        return Geometry(packed_rows(conv_size(2 * s[0] - 1)), 1, s[0], 2, s[0], 2, 0)
    if f == "czt":
        return Geometry(packed_rows(conv_size(s[0] + s[1] - 1)), 1, s[0], 2, s[1], 2, 0)
    if f == "dwt":
        n, levels, key = s
        return Geometry(1, dwt_tiles(DWT_TAPS[key], levels, n, c.dt, c.op == "inverse")[1], n, 1, n, 1, 0)
    if f == "upfirdn":
        up, down, ntaps, n = s
        y_len = upfirdn_output_len(n, up, down, ntaps)
        return Geometry(1, upfirdn_tiles(up, down, ntaps, y_len, c.dt), n, 1, y_len, 1, 0)
    if f == "sdft":
        n, t, hop, _ = s
        frames_out = 1 + (t - n) // hop
        return Geometry(1, sdft_blocks_per_row(n, t, SDFT_BINS, c.dt), t, 1, SDFT_BINS * frames_out, 2, 0)
    if f == "ntt":
        n = 1 << s[0]
        return Geometry(ntt_rows(s[0], c.op), 1, n, 2 if c.op == "convolve" else 1, n, 1, 0)
    raise ValueError(f)


def stride_of(c, v):
    """The row stride of rows of v values: v itself, or in the padded variants the next multiple of 16 bytes beyond v
    (fast), or the second odd number beyond v - 1 (odd; there the rows begin one element into the buffer)."""
    q = 16 // ELEM[c.dt]
    return {"fast": (v // q + 1) * q, "odd": v + 3 - v % 2}.get(c.variant, v)


def rows_of(c, cus):
    """B: the rows of the big batch."""
    w = ROUNDS * cus
    g = geometry(c)
    if g.r > 1:
        b = -(-(w * g.r + g.r // 2 + 1) // g.per_row)
        while (b * g.per_row) % g.r == 0:
            b += 1
    else:
        b = max(-(-w // g.per_row), K + 1)
    if c.family == "istft" and c.dt == "f64" and c.shape[0] == 16384 and c.shape[1] < c.shape[0]:
        b = max(b, 3 * istft_chunk_frames(c.shape[0], c.shape[1], 1 << 40, 8) + 1)  # four chunks at least
    if c.line:  # the f64 planes pass 2^32 bytes; the f32 run at the same B passes 2^31
        b = max(b, -(-LINE["f64"] // (min(g.vin, g.vout) * 8)) + K)
    return b


def workgroups(c, b):
    g = geometry(c)
    return -(-(b * g.per_row) // g.r)


def bytes_in_out(c, b):
    g = geometry(c, b)
    es = ELEM[c.dt]
    bin_ = b * stride_of(c, g.vin) * g.pin * es
    if c.family == "stft":
        bin_ = (b - 1 + c.shape[0] // c.shape[1]) * c.shape[1] * es
    bout = 0 if c.variant == "inplace" else b * stride_of(c, g.vout) * g.pout * es
    if c.family == "istft":
        bout = ((b - 1) * c.shape[1] + c.shape[0]) * es
    return bin_, bout


def live_bytes(c, b):
    """Inputs, outputs and the call's scratch, the 61-row reference, and the comparison's temporaries (a mask of one
    slice and, on a mismatch only, nothing larger)."""
    g = geometry(c, b)
    bin_, bout = bytes_in_out(c, b)
    ref = 3 * K * (g.vin * g.pin + g.vout * g.pout) * ELEM[c.dt]
    tiled_copy = b * g.vin * ELEM[c.dt] if c.variant in ("fast", "odd") else 0  # the padded input is filled from a tiled temporary
    return bin_ + bout + g.extra + ref + tiled_copy + 2 * SLICE


def locate(c, row):
    """(workgroup, slot) of a row's first work item."""
    g = geometry(c)
    return (row * g.per_row) // g.r, (row * g.per_row) % g.r


# ---- the table ------------------------------------------------------------------------------------------------------

PACKED_NS = (64, 2048, 16384)  # 128 rows per workgroup; M / 16 = 64, where uniform_row turns to readfirstlane; one
MID_N = 2048                   # 512-thread workgroup per row
DFT_LS = (2, 1000, 4096)                         # M = 32, 2048, 8192
CZT_SHAPES = ((11, 22), (700, 1000), (4096, 4096))  # M = 32, 2048, 8192
DWT_SHAPES = ((96, 5, "db2"), (4096, 12, "db4"), (12288, 4, "db2"), (98304, 8, "db8"))  # resident x 2, tiled x 2
UPFIRDN_SHAPES = ((5, 1, 8, 64), (3, 2, 17, 300))  # (up, down, taps, len): the ends of test_gpu_resample_paths.FORCED
SDFT_SHAPES = ((2, 13, 1, "rect"), (16384, 3 * 16384 + 7, 1, "blackman"))  # the ends of sdft_ref.PATH_SIZES
NTT_LOG2 = (6, 14)


def _plain():
    out = []
    for dt in DTS:
        for n in PACKED_NS:
            out += [Case("dct", t, dt, (n,), None, False) for t in (2, 3)]
            out += [Case("hilbert", m, dt, (n,), None, False) for m in ("analytic", "envelope")]
            out.append(Case("fir", None, dt, (n,), None, False))
            for fam in ("stft", "istft"):
                out.append(Case(fam, None, dt, (n, n // 4), None, False))
        for fam in ("stft", "istft"):
            out.append(Case(fam, None, dt, (MID_N, MID_N), None, False))  # hop = N: the direct inverse
        for ln in DFT_LS:
            out += [Case("dft", op, dt, (ln,), None, False) for op in ("forward", "inverse")]
        out += [Case("czt", None, dt, s, None, False) for s in CZT_SHAPES]
        for s in DWT_SHAPES:
            if s[0] == 12288 and dt == "f64":
                continue  # the f32 row one above the resident threshold
            out += [Case("dwt", op, dt, s, None, False) for op in ("forward", "inverse")]
        out += [Case("upfirdn", None, dt, s, None, False) for s in UPFIRDN_SHAPES]
        out += [Case("sdft", None, dt, s, None, False) for s in SDFT_SHAPES]
    for lg in NTT_LOG2:
        out += [Case("ntt", op, "u64", (lg,), None, False) for op in ("forward", "inverse", "convolve")]
    return out


def _lines():
    """The single-plane real-row families at their largest row, past 2^31 (f32) and 2^32 (f64) bytes."""
    out = []
    for dt in DTS:
        out.append(Case("dct", 2, dt, (16384,), None, True))
        out.append(Case("fir", None, dt, (16384,), None, True))
        out.append(Case("dwt", "forward", dt, DWT_SHAPES[-1], None, True))
        out.append(Case("upfirdn", None, dt, UPFIRDN_SHAPES[-1], None, True))
    return out


def _variants():
    """The middle shape of each family with a layout of its own: in place, 16-byte padded strides, odd strides."""
    out = []
    for dt in DTS:
        mids = [Case("dct", 2, dt, (MID_N,), None, False), Case("hilbert", "envelope", dt, (MID_N,), None, False),
                Case("dft", "forward", dt, (DFT_LS[1],), None, False), Case("dwt", "forward", dt, DWT_SHAPES[1], None, False)]
        out += [c._replace(variant="inplace") for c in mids]
        # Czt writes K bins per row of L samples: only L = K has an in-place call, the largest shape here
        out.append(Case("czt", None, dt, CZT_SHAPES[2], "inplace", False))
        strided = mids[:1] + [Case("hilbert", "analytic", dt, (MID_N,), None, False), Case("fir", None, dt, (MID_N,), None, False),
                              mids[2], Case("czt", None, dt, CZT_SHAPES[1], None, False), mids[3],
                              Case("upfirdn", None, dt, UPFIRDN_SHAPES[1], None, False)]  # two shapes: the larger
        out += [c._replace(variant=v) for c in strided for v in ("fast", "odd")]
    return out


PLAIN, LINES, VARIANTS = _plain(), _lines(), _variants()


# ---- the periodic signal of the STFT cases ------------------------------------------------------------------------------

def periodic_signal(base, frames, n):
    """base [K, hop] -> the signal of `frames` frames of n samples at hop base.shape[1] whose period is K hops."""
    import numpy as np
    k, hop = base.shape
    hops = frames - 1 + n // hop
    return base[np.arange(hops) % k].reshape(-1)


# ---- the comparison ---------------------------------------------------------------------------------------------------

def first_mismatch(out, ref, slice_elems=SLICE):
    """out [B, C] and ref [k, C], integer tensors on one device (out's rows may sit at a stride): None where row r of
    out equals row r mod k of ref everywhere, else (row, column, got, want) of the first difference.  Whole groups are
    compared in slices of at most slice_elems elements, then the remainder with ref[:rem]."""
    import torch
    b, c = out.shape
    k = ref.shape[0]
    groups = b // k
    per = max(1, slice_elems // (k * c))
    spans = [(g0 * k, min(groups, g0 + per) * k) for g0 in range(0, groups, per)]
    if b > groups * k:
        spans.append((groups * k, b))
    for lo, hi in spans:
        if hi - lo >= k:
            ne = out[lo:hi].unflatten(0, ((hi - lo) // k, k)) != ref
        else:
            ne = out[lo:hi] != ref[:hi - lo]
        if bool(ne.any()):
            i = int(ne.reshape(-1).view(torch.uint8).argmax())
            row, col = lo + i // c, i % c
            return row, col, int(out[row, col]), int(ref[row % k, col])
    return None


def describe(c, row, col, got, want):
    wg, slot = locate(c, row)
    bits = 8 * ELEM[c.dt]
    mask = (1 << bits) - 1
    return (f"first difference at row {row} (base row {row % K}), workgroup {wg}, slot {slot}, column {col}: "
            f"got {got & mask:#0{bits // 4 + 2}x}, want {want & mask:#0{bits // 4 + 2}x}")

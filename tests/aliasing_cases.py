"""The rows of tests/test_gpu_aliasing.py and what tests/test_aliasing_table_cpu.py checks about them: no GPU, no torch
at import.

DESIGN.md 4.1d states the aliasing contract of the single-pass transforms and of the spectra; include/pdsp_hip.h
repeats it at the entry points.  One row per (entry point, dtype, kernel reached): `kernel` is a name of the path
vocabulary of test_gpu_f32_paths.expected_path / test_gpu_f64_paths.expected_path_f64 (a prefix for the spectrum
kernels, whose names carry the instantiation), and the GPU module asserts it on the library's own answer
(pdsp_dev_transform_path_* / pdsp_dev_spectrum_path_*) before every call.

Batches: the smallest with at least three workgroups and a partial last one, 2 x rows-per-workgroup + 1 (3 rows where
a workgroup holds one row; fft_real_kernel at N = 16384 takes 8 rows, the batch from which the dispatch picks it).
"""
import os
import re
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pdsp_hip.h")

# kind: complex / real / inverse / ifwd / iinv.  offs: misalignment of (re_in, im_in, re_out, im_out) in elements
# (interleaved: of in and out, in scalars).  switches: the development switches the row runs under.
TRow = namedtuple("TRow", "name entry kind dt n batch offs switches kernel")
# outputs: a subset of amp / ph / idx / rec.  window: None, ("plan", kind) or ("table", kind).  stride: frame_stride
# (below n: overlapping frames of one signal).
SRow = namedtuple("SRow", "name entry dt n batch stride window sides outputs kernel")

DTS = ("f32", "f64")
ENTRY = {"complex": "pdsp_fft_forward_complex", "real": "pdsp_fft_forward_real", "inverse": "pdsp_fft_inverse",
         "ifwd": "pdsp_fft_forward_interleaved", "iinv": "pdsp_fft_inverse_interleaved"}
PLANAR = ("complex", "real", "inverse")


def rows_per_workgroup(kernel, n):
    """Rows of N points one workgroup of `kernel` holds (pdsp_fft_core.h: FftTraits, the 4096-point chunks of the
    staged kernels, the packed-real rows of N / 2 points)."""
    if kernel in ("fft_tiny_staged_kernel", "fft_staged_kernel", "fft_tiny_staged_kernel<AMP>"):
        return 4096 // n
    if kernel == "spectrum_staged_kernel":
        return 4096 // (n // 2)
    if kernel.startswith("spectrum_packed_kernel"):
        return max(256 // max(n // 2 // 16, 1), 1)
    if kernel in ("fft_stockham_kernel", "small-complex-(x,0)"):
        return max(256 // max(n // 16, 1), 1)
    return 1  # fft_split2_kernel, fft_split4_kernel, fft_real_kernel, spectrum_dif16k_kernel: one row


def batch_of(kernel, n):
    return 2 * rows_per_workgroup(kernel, n) + 1


ALIGNED = (0, 0, 0, 0)
OFF16 = (1, 3, 2, 1)   # no plane on a 16-byte (f32) or 32-byte (f64) boundary
# (kernel, N, offsets, switches, kinds or None for all three) by dtype
TRANSFORM_SPECS = {
    "f32": [
        ("fft_tiny_staged_kernel", 2, ALIGNED, None, None),
        ("fft_tiny_staged_kernel", 16, ALIGNED, None, None),
        ("fft_stockham_kernel", 1, ALIGNED, None, None),
        ("fft_stockham_kernel", 8, OFF16, None, None),
        ("fft_stockham_kernel", 64, ALIGNED, {"staged_small": 0}, None),
        ("fft_stockham_kernel", 512, ALIGNED, None, None),
        ("fft_stockham_kernel", 4096, ALIGNED, None, None),
        ("fft_stockham_kernel", 8192, (2, 0, 0, 0), None, None),
        ("fft_stockham_kernel", 16384, (2, 0, 0, 0), None, None),
        ("fft_staged_kernel", 32, ALIGNED, None, None),
        ("fft_staged_kernel", 256, ALIGNED, None, None),
        ("fft_split2_kernel", 8192, ALIGNED, None, ("real",)),
        ("fft_split4_kernel", 16384, ALIGNED, None, None),
    ],
    "f64": [
        ("fft_tiny_staged_kernel", 2, ALIGNED, None, None),
        ("fft_tiny_staged_kernel", 16, ALIGNED, None, None),
        ("fft_stockham_kernel", 1, ALIGNED, None, None),
        ("fft_stockham_kernel", 8, OFF16, None, None),
        ("fft_stockham_kernel", 64, ALIGNED, {"staged_small": 0}, None),
        ("fft_stockham_kernel", 512, ALIGNED, None, None),
        ("fft_stockham_kernel", 4096, ALIGNED, None, None),
        ("fft_stockham_kernel", 8192, (1, 0, 0, 0), None, None),
        ("fft_staged_kernel", 32, ALIGNED, None, None),
        ("fft_staged_kernel", 128, ALIGNED, None, None),
        ("fft_split2_kernel", 8192, ALIGNED, None, ("complex", "inverse")),
        ("fft_real_kernel", 8192, ALIGNED, None, ("real",)),
        ("fft_real_kernel", 16384, ALIGNED, None, ("real",)),
    ],
}
INTERLEAVED_N = {"f32": (1, 64, 4096, 16384), "f64": (1, 64, 4096, 8192)}


def _transform_rows():
    out = []
    for dt in DTS:
        for kernel, n, offs, sw, kinds in TRANSFORM_SPECS[dt]:
            for kind in kinds or PLANAR:
                batch = 8 if (kernel, n) == ("fft_real_kernel", 16384) else batch_of(kernel, n)
                tag = "-".join(f"{k}{v}" for k, v in (sw or {}).items())
                name = f"{kind}-{dt}-{kernel}-{n}" + ("-off" if any(offs) else "") + (f"-{tag}" if tag else "")
                out.append(TRow(name, f"{ENTRY[kind]}_{dt}", kind, dt, n, batch, offs, sw, kernel))
        for n in INTERLEAVED_N[dt]:
            for kind in ("ifwd", "iinv"):
                out.append(TRow(f"{kind}-{dt}-fft_stockham_kernel-{n}", f"{ENTRY[kind]}_{dt}", kind, dt, n,
                                batch_of("fft_stockham_kernel", n), (0, 0, 0, 0), None, "fft_stockham_kernel"))
    return out


A, P, I, R = ("amp",), ("amp", "ph"), ("amp", "idx"), ("rec",)
S, SP = "pdsp_spectrum", "pdsp_spectrum_peaks_f32"
# (tag, entry stem, dtype, kernel prefix, N, stride or None, window, sides, outputs)
SPECTRUM_SPECS = [
    ("tiny", S, "f32", "fft_tiny_staged_kernel<AMP>", 16, None, ("table", "hann"), "one", A),
    ("tiny", S, "f64", "fft_tiny_staged_kernel<AMP>", 16, None, None, "two", A),
    ("x0", S, "f32", "small-complex-(x,0)", 32, None, ("table", "hamming"), "two", ("amp", "ph", "idx")),
    ("x0", S, "f64", "small-complex-(x,0)", 32, None, None, "one", ("amp", "ph", "idx")),
    ("staged", S, "f32", "spectrum_staged_kernel", 64, None, ("table", "hann"), "one", A),
    ("staged", S, "f32", "spectrum_staged_kernel", 512, None, None, "one", A),
    ("fast-rect", S, "f32", "spectrum_packed_kernel-FAST-m9-w0", 1024, None, None, "one", I),
    ("fast-table", S, "f32", "spectrum_packed_kernel-FAST-m10-w1", 2048, None, ("table", "blackman"), "one", A),
    ("fast-fused", S, "f32", "spectrum_packed_kernel-FAST-m11-w2", 4096, None, ("plan", "hann"), "one", A),
    ("general-two", S, "f32", "spectrum_packed_kernel-general-m7-w1", 256, None, ("table", "hann"), "two", P),
    ("hop", S, "f32", "spectrum_packed_kernel-FAST-m9-w2", 1024, 256, ("plan", "hamming"), "one", I),
    ("fast", S, "f64", "spectrum_packed_kernel-FAST-m9-w1", 1024, None, ("table", "hann"), "one", I),
    ("general-two", S, "f64", "spectrum_packed_kernel-general-m7-w0", 256, None, None, "two", P),
    ("hop", S, "f64", "spectrum_packed_kernel-general-m9-w1", 1024, 257, ("plan", "hann"), "one", ("amp", "ph", "idx")),
    ("dif16k", S, "f32", "spectrum_dif16k_kernel-w3", 16384, None, ("plan", "blackman"), "one", I),
    ("peaks-wave", SP, "f32", "small-complex-(x,0)", 32, None, None, "one", ("rec", "amp", "ph")),
    ("peaks-fused-packed", SP, "f32", "spectrum_packed_kernel-FAST-m9-w0-peak", 1024, None, None, "one", ("rec", "amp")),
    ("peaks-fused-two", SP, "f32", "spectrum_packed_kernel-general-m9-w1-peak", 1024, None, ("table", "hann"), "two",
     ("rec", "amp", "ph")),
    ("peaks-fused-dif16k", SP, "f32", "spectrum_dif16k_kernel-w1-peak", 16384, None, ("table", "hann"), "one",
     ("rec", "amp")),
    ("peaks-hop", SP, "f32", "spectrum_packed_kernel-FAST-m9-w0-peak", 1024, 512, None, "one", R),
]


def _spectrum_rows():
    out = []
    for tag, stem, dt, kernel, n, stride, window, sides, outputs in SPECTRUM_SPECS:
        entry = stem if stem == SP else f"{stem}_{dt}"
        base = kernel.split("-")[0] if kernel.startswith("spectrum_") else kernel
        out.append(SRow(f"spectrum-{tag}-{dt}-{n}", entry, dt, n, batch_of(base, n), stride or n, window, sides,
                        tuple(outputs), kernel))
    return out


TRANSFORM_ROWS = _transform_rows()
SPECTRUM_ROWS = _spectrum_rows()
ROWS = TRANSFORM_ROWS + SPECTRUM_ROWS

# What the issue of this table asks the rows to reach: (kernel, dtype) -> sizes
REQUIRED_TRANSFORMS = {
    ("fft_tiny_staged_kernel", "f32"): {2, 16}, ("fft_tiny_staged_kernel", "f64"): {2, 16},
    ("fft_stockham_kernel", "f32"): {1, 8, 64, 512, 4096, 8192, 16384},
    ("fft_stockham_kernel", "f64"): {1, 8, 64, 512, 4096, 8192},
    ("fft_staged_kernel", "f32"): {32, 256}, ("fft_staged_kernel", "f64"): {32, 128},
    ("fft_split2_kernel", "f32"): {8192}, ("fft_split2_kernel", "f64"): {8192},
    ("fft_split4_kernel", "f32"): {16384},
    ("fft_real_kernel", "f64"): {8192, 16384},
}
REQUIRED_SPECTRUM_PREFIXES = (
    "fft_tiny_staged_kernel<AMP>", "small-complex-(x,0)", "spectrum_staged_kernel", "spectrum_packed_kernel-FAST",
    "spectrum_packed_kernel-general", "spectrum_dif16k_kernel",
)


def declared_entries():
    return {r.entry for r in ROWS}


def aliasing_entry_points(path=HEADER):
    """The device entry points of the two oldest families in the header, comments stripped, in header order: every
    pdsp_fft_*_f32 / _f64 and every pdsp_spectrum* that takes a stream (the *_host_* forms stage through buffers of
    their own and keep their own overlap rule)."""
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = []
    for name, args in re.findall(r"\bPDSP_API\s+[\w\s\*]*?\b(pdsp_\w+)\s*\(([^;{}]*?)\)\s*;", text):
        if not " ".join(args.split()).endswith("pdsp_stream stream") or "_host_" in name:
            continue
        if re.fullmatch(r"pdsp_fft_\w+_f(32|64)", name) or name.startswith("pdsp_spectrum"):
            out.append(name)
    return out

"""The rows of tests/test_gpu_graph_capture.py and what tests/test_graph_capture_table_cpu.py checks about them: no
GPU, no torch at import.

DESIGN.md, "Streams and graphs", states the contract: a device entry point that draws no stream-ordered scratch, on a
handle that has made one eager call in the precision, makes only kernel launches on the stream it is given, so it can
be captured into a graph and replayed.  Every function of include/pdsp_hip.h whose last parameter is `pdsp_stream
stream` is an entry point of that contract; each appears in the `entries` of at least one row below, and the GPU test
asserts, through a recording proxy of the library, that a row reaches exactly the entry points it declares.

A row: name (the test id), family (which builder of the GPU module makes the handle, the inputs and the call), op, dt
("f32", "f64", "u64"), shape (the family's own tuple) and entries.  Shapes are the smallest at which each kernel form is
still itself: N = 64 in 5 rows (a workgroup holds several rows there, so the last one has dead rows) and N = 4096 in 3.
"""
import os
import re
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pdsp_hip.h")

Row = namedtuple("Row", "name family op dt shape entries")

DTS = ("f32", "f64")
SIZES = ((64, 5), (4096, 3))       # (N, rows) of the transforms and the packed-real families
SPECTRUM_16K = (16384, 3)          # f32, a named window: the fused cosine-sum form of spectrum_dif16k_kernel
DFT_LENGTHS = ((17, 5), (1000, 3))  # (L, rows): M = 64 and 2048
CZT_SHAPE = (100, 37, 3)            # (L, K, rows) of the zoom case, on test_gpu_czt's grid step and start
RESAMPLE = (3, 2, 300, 3)           # (up, down, row length, rows), the default taps
UPFIRDN = (3, 2, 17, 300, 3)        # (up, down, taps, row length, rows), the caller's taps
DWT = ("db4", 3, 256, 3)            # (wavelet, levels, row length, rows)
NTT_SIZES = ((64, 5), (4096, 3))
SDFT = (64, (0.0, 12.5, 31.0), 1, 200, 3)  # (window, bins, hop, samples, rows)
FIR = {64: (9, 100), 4096: (33, 5000)}     # block -> (taps, row length): several blocks per row


def fir_spectrum_taps(n):
    """The taps of the filter-spectrum rows: N / 2, the longest filter of a block.  The family's f64 bound
    (test_gpu_fir_paths.SPEC_TOL_F64[N] x sum|h|) is measured there; it is no bound for a short filter, where the
    rounding of one product alone, 2^-53 |h_j|, is a larger share of sum|h| (measured at 33 taps, N = 4096: 9.8e-17
    against 7e-17)."""
    return n // 2


ELEMENTWISE = (3, 1001)             # (rows, row length): odd, so the last workgroup is partial
COMPLEX_OPS = ("add", "sub", "mul", "div", "conj", "scale", "mulScalar")  # every code of pdsp_complex_op_f32
SPECTRUM_VARIANTS = ("amp", "amp-phase-peak", "named", "table", "two")

# Forms of a call that are outside the contract ("Streams and graphs"): they draw stream-ordered scratch
# (hipMallocFromPoolAsync, StreamScratch) or only clear their outputs (hipMemsetAsync, no kernel).  No row captures them.
SCRATCH = "draws stream-ordered scratch"
CLEAR = "clear-only degenerate path"
EXCLUDED_FORMS = (
    ("pdsp_fft_*", "a transform beyond the single-pass size (run_complex with scratch plane pairs)", SCRATCH),
    ("pdsp_spectrum_*", "a spectrum on a multi-pass path, or peak records without the amplitude and phase rows where the "
                        "peaks are not fused (spectrum_impl: pairs or peak_rows_extra)", SCRATCH),
    ("pdsp_istft_*", "hop < N, the overlapped two-pass inverse", SCRATCH),
    ("pdsp_spectrum_*", "frame_len == 0 (kSpecMemset)", CLEAR),
    ("pdsp_fir_filter_*", "len == 0", CLEAR),
)
# Whole entry points no row could reach: none.  Every stream entry point has a scratch-free form.
EXCLUDED = {}


def _e(stem, dt):
    return (f"pdsp_{stem}_{dt}",)


def _rows():
    out = []

    def add(name, family, op, dt, shape, entries):
        out.append(Row(name, family, op, dt, shape, tuple(entries)))

    for dt in DTS:
        for n, rows in SIZES:
            tag = f"{n}x{rows}-{dt}"
            add(f"fft-forward-real-{tag}", "fft", "real", dt, (n, rows), _e("fft_forward_real", dt))
            add(f"fft-forward-complex-{tag}", "fft", "complex", dt, (n, rows), _e("fft_forward_complex", dt))
            add(f"fft-inverse-{tag}", "fft", "inverse", dt, (n, rows), _e("fft_inverse", dt))
            add(f"fft-forward-interleaved-{tag}", "fft", "ifwd", dt, (n, rows), _e("fft_forward_interleaved", dt))
            add(f"fft-inverse-interleaved-{tag}", "fft", "iinv", dt, (n, rows), _e("fft_inverse_interleaved", dt))
            for v in SPECTRUM_VARIANTS:
                add(f"spectrum-{v}-{tag}", "spectrum", v, dt, (n, rows), _e("spectrum", dt))
            add(f"stft-{tag}", "stft", "amp", dt, (n, rows), _e("spectrum", dt))
            add(f"stft-complex-{tag}", "stft", "complex", dt, (n, rows), _e("stft_complex", dt))
            add(f"istft-{tag}", "istft", None, dt, (n, rows), _e("istft", dt))
            for op in ("dct", "idct"):
                for t in (2, 3):
                    for layout in ("fast", "general"):
                        add(f"{op}{t}-{layout}-{tag}", "dct", (op, t, layout), dt, (n, rows), _e("dct", dt))
            for mode in ("analytic", "imag", "envelope", "phase"):
                add(f"hilbert-{mode}-{tag}", "hilbert", mode, dt, (n, rows), _e("hilbert", dt))
            add(f"fir-apply-{tag}", "fir", "apply", dt, (n, rows), _e("fir_filter", dt))
            add(f"fir-spectrum-{tag}", "fir", "spectrum", dt, (n, rows), _e("fir_spectrum", dt))
        for ln, rows in DFT_LENGTHS:
            for op in ("forward", "inverse"):
                add(f"dft-{op}-{ln}x{rows}-{dt}", "dft", op, dt, (ln, rows), _e("dft_c2c", dt))
        add(f"czt-zoom-{dt}", "czt", None, dt, CZT_SHAPE, _e("czt", dt))
        add(f"resampler-{dt}", "resample", "poly", dt, RESAMPLE, _e("upfirdn", dt))
        add(f"upfirdn-{dt}", "resample", "upfirdn", dt, UPFIRDN, _e("upfirdn", dt))
        for op in ("forward", "inverse"):
            add(f"dwt-{op}-{dt}", "dwt", op, dt, DWT, _e(f"dwt_{op}", dt))
        add(f"sdft-{dt}", "sdft", None, dt, SDFT, _e("sdft", dt))
        add(f"apply-window-{dt}", "elementwise", "apply_window", dt, ELEMENTWISE, _e("apply_window", dt))
        add(f"magnitude-{dt}", "elementwise", "magnitude", dt, ELEMENTWISE, _e("magnitude", dt))
        add(f"phase-{dt}", "elementwise", "phase", dt, ELEMENTWISE, _e("phase", dt))
    add("spectrum-named-16384x3-f32", "spectrum", "named", "f32", SPECTRUM_16K, _e("spectrum", "f32"))
    for n, rows in SIZES:
        add(f"spectrum-peaks-{n}x{rows}-f32", "peaks", None, "f32", (n, rows), ("pdsp_spectrum_peaks_f32",))
    for op in COMPLEX_OPS:
        add(f"complex-{op}-f32", "complex", op, "f32", ELEMENTWISE, ("pdsp_complex_op_f32",))
    for n, rows in NTT_SIZES:
        add(f"ntt-forward-{n}x{rows}", "ntt", "forward", "u64", (n, rows), ("pdsp_ntt_forward_u64",))
        add(f"ntt-inverse-{n}x{rows}", "ntt", "inverse", "u64", (n, rows), ("pdsp_ntt_inverse_u64",))
        add(f"ntt-convolve-{n}x{rows}", "ntt", "convolve", "u64", (n, rows), ("pdsp_ntt_conv_u64",))
    add("ntt-mul", "ntt", "mul", "u64", (64, 5), ("pdsp_ntt_mul_u64",))
    return out


ROWS = _rows()
IDS = [r.name for r in ROWS]


def declared_entries():
    return {e for r in ROWS for e in r.entries}


def stream_entry_points(path=HEADER):
    """Every function of the header whose last parameter is `pdsp_stream stream`, comments stripped, in header order."""
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = []
    for name, args in re.findall(r"\bPDSP_API\s+[\w\s\*]*?\b(pdsp_\w+)\s*\(([^;{}]*?)\)\s*;", text):
        if " ".join(args.split()).endswith("pdsp_stream stream"):
            out.append(name)
    return out

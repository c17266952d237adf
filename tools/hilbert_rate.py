#!/usr/bin/env python3
"""Rates of the Hilbert kernel on the GPU: BatchedFft.hilbert / hilbert_imag / envelope / instantaneous_phase (one
fused launch per call, pdsp_hilbert_kernel.h) against two yardsticks timed in the same process on the same inputs:
the same result composed in torch (torch.fft.rfft, the -i mask, irfft, the element-wise tail; outputs compared) and
fir_overlap_save_kernel with a short filter (N/16 - 1 taps) at the same N, which does the same two transforms per
block.  The Hilbert kernel is timed on its FAST path and, with len = N - 2, on its general path; the FIR kernel on
its FAST instantiation (mode "filter") and on its general one (mode "same"); which one a call takes is asserted from
a mirror of the library's condition.  f32 and f64, N = 1024 / 4096 / 16384, 2^26 samples per call.  Device events;
per function 5 warm-up calls, then --windows windows of about --window-s seconds each, the functions alternating
window by window; min / median / max of the windows are recorded and the ratios use the medians.  Prints one JSON
line per case: GSample/s (per output sample), algorithmic TB/s (N sizeof T in plus N or 2N out per row: what a call
must move, not what it moves), its share of 8 TB/s, and the ratios.

    python tools/hilbert_rate.py [--out profiles/hilbert_rate.jsonl] [--samples-log2 26] [--window-s 0.15]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pragma_dsp_amd.batch import BatchedFft  # noqa: E402
from pragma_dsp_amd.filters import FirFilter, output_range  # noqa: E402

PEAK_TBPS = 8.0
MODES = ("analytic", "imag", "envelope", "phase")


def window(fn, iters):
    """Seconds per call over one window of `iters` calls (device events)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def timed_together(fns, window_s, windows):
    """Each fn of the dict: 5 warm-up calls, an iteration count that fills a window of `window_s` seconds, then
    `windows` windows, the fns alternating window by window.  Returns {name: (min, median, max) seconds per call}."""
    iters = {}
    for k, fn in fns.items():
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        iters[k] = max(20, int(window_s / max(window(fn, 20), 1e-6)))
    got = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            got[k].append(window(fn, iters[k]))
    return {k: (min(v), statistics.median(v), max(v)) for k, v in got.items()}


def torch_hilbert(x, mode):
    """The same result in torch ops: rfft, -i on bins 1 ... N/2 - 1, zeros at DC and Nyquist, irfft, the tail."""
    n = x.shape[1]
    X = torch.fft.rfft(x, dim=1)
    Y = X * (-1j)
    Y[:, 0] = 0
    Y[:, n // 2] = 0
    h = torch.fft.irfft(Y, n=n, dim=1)
    if mode == "analytic":
        return torch.complex(x, h)
    if mode == "imag":
        return h
    if mode == "envelope":
        return torch.sqrt(x * x + h * h)
    return torch.atan2(h, x)


def run(plan, x, mode, out):
    return {"analytic": plan.hilbert, "imag": plan.hilbert_imag, "envelope": plan.envelope,
            "phase": plan.instantaneous_phase}[mode](x, out=out)


def fir_is_fast(fir, x, y, mode):
    """Mirror of fir_filter_dev's fast-path condition (pdsp_kernels_fir.hip)."""
    y_off, _ = output_range(x.shape[-1], fir.ntaps, mode)
    p = fir.ntaps if fir.ntaps % 2 else fir.ntaps + 1
    hop = fir.size - (p - 1)
    es = x.element_size()
    return ((x.data_ptr() | y.data_ptr()) % 8 == 0 and x.shape[-1] % 2 == 0 and y.shape[-1] % 2 == 0 and hop % 2 == 0
            and (y_off - (p - 1)) % 2 == 0 and es in (4, 8))


def ms3(t):
    return [round(v * 1e3, 4) for v in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples-log2", type=int, default=26)
    ap.add_argument("--window-s", type=float, default=0.15)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--modes", default=",".join(MODES))
    ap.add_argument("--sizes", default="1024,4096,16384")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    for dname in args.dtypes.split(","):
        dtype = torch.float32 if dname == "f32" else torch.float64
        esize = 4 if dtype == torch.float32 else 8
        cdt = torch.complex64 if esize == 4 else torch.complex128
        for n in (int(v) for v in args.sizes.split(",")):
            plan = BatchedFft(n, dev, dtype)
            rows = (1 << args.samples_log2) // n
            samples = rows * n
            x = torch.randn((rows, n), device=dev, dtype=dtype)
            # the FIR yardstick: one long row of the same samples, N/16 - 1 taps (odd), as many outputs as inputs.
            # Mode "filter" (outputs from 0) runs fir_overlap_save_kernel's FAST instantiation, mode "same" (outputs
            # from (P - 1) / 2, odd against P - 1) its general one; both are timed and named.
            fir = FirFilter(torch.randn(n // 16 - 1).numpy(), dev, dtype, block=n)
            xl = x.view(1, samples)
            yl = torch.empty_like(xl)
            assert fir_is_fast(fir, xl, yl, "filter") and not fir_is_fast(fir, xl, yl, "same")
            # the general path of the Hilbert kernel: the same rows with len = N - 2 (zero-padded to N)
            xg = x[:, :n - 2]
            for mode in args.modes.split(","):
                y = torch.empty((rows, n), device=dev, dtype=cdt if mode == "analytic" else dtype)
                run(plan, x, mode, y)
                want = torch_hilbert(x, mode)
                if mode == "phase":  # weighted by the sample's size, wrapped (tests/test_gpu_hilbert.py)
                    a = torch.sqrt(x * x + torch_hilbert(x, "imag") ** 2)
                    dphi = torch.remainder(y - want + torch.pi, 2 * torch.pi) - torch.pi
                    err = (dphi.abs() * a / a.amax(dim=1, keepdim=True)).max().item()
                    del a, dphi
                else:
                    den = torch_hilbert(x, "analytic").abs().amax(dim=1, keepdim=True)
                    err = ((y - want).abs() / den).max().item()
                    del den
                del want
                t = timed_together({
                    "hilbert": lambda: run(plan, x, mode, y),
                    "hilbert_general": lambda: run(plan, xg, mode, y),
                    "fir_fast": lambda: fir.apply(xl, "filter", out=yl),
                    "fir_general": lambda: fir.apply(xl, "same", out=yl),
                    "torch": lambda: torch_hilbert(x, mode),
                }, args.window_s, args.windows)
                t_k = t["hilbert"][1]
                moved = samples * esize * (3 if mode == "analytic" else 2)
                tbps = moved / t_k / 1e12
                rec = {"dtype": dname, "n": n, "mode": mode, "rows": rows, "samples": samples,
                       "hilbert_ms_min_med_max": ms3(t["hilbert"]), "hilbert_gsps": round(samples / t_k / 1e9, 2),
                       "hilbert_tbps": round(tbps, 3), "pct_of_8tbps": round(100 * tbps / PEAK_TBPS, 1),
                       "torch_ms_min_med_max": ms3(t["torch"]), "vs_torch": round(t["torch"][1] / t_k, 2),
                       "fir_fast_ms_min_med_max": ms3(t["fir_fast"]),
                       "fir_fast_gsps": round(samples / t["fir_fast"][1] / 1e9, 2),
                       "vs_fir_fast": round(t["fir_fast"][1] / t_k, 3),
                       "fir_general_ms_min_med_max": ms3(t["fir_general"]),
                       "hilbert_general_ms_min_med_max": ms3(t["hilbert_general"]),
                       "general_vs_fast": round(t["hilbert_general"][1] / t_k, 3),
                       "general_vs_fir_general": round(t["fir_general"][1] / t["hilbert_general"][1], 3),
                       "max_diff_vs_torch": float(f"{err:.3e}")}
                print(json.dumps(rec), flush=True)
                lines.append(rec)
                del y
            del x, xl, xg, yl, fir
            torch.cuda.empty_cache()
            plan.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

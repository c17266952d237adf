#!/usr/bin/env python3
"""Rates of the any-length DFT on the GPU: Dft.forward (one fused chirp-z launch per call, pdsp_bluestein_kernel.h)
against two yardsticks timed in the same process:

  torch    torch.fft.fft on the same rows as one complex tensor (rocFFT; outputs compared);
  hilbert  hilbert_kernel, IMAG mode, general path (len = N - 2), at N = 2M on the same number of rows: the same two
           pass sets of M points, the same LDS and the same occupancy class, so its rows per second are what the
           chirp-z kernel should approach per workgroup.

L = 1000, 1920, 4095, 4096, f32 and f64, forward, 2^26 complex samples per call.  Device events; per function
--warmup calls, then --calls timed calls, the functions alternating call by call; min / median / max are recorded and
the ratios use the medians.  Prints one JSON line per case: GSample/s (complex samples), algorithmic TB/s (2 sizeof T
in plus 2 sizeof T out per sample: what a call must move), rows per second of both kernels, and the ratios.

    python tools/dft_rate.py [--out profiles/dft_rate.jsonl] [--samples-log2 26]
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
from pragma_dsp_amd.dft import Dft  # noqa: E402

PEAK_TBPS = 8.0


def timed_together(fns, warmup, calls):
    """Each fn of the dict: `warmup` calls, then `calls` timed calls (device events around each), the fns alternating
    call by call.  Returns {name: (min, median, max) seconds per call}."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in fns}
    for _ in range(calls):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            got[k].append(e0.elapsed_time(e1) * 1e-3)
    return {k: (min(v), statistics.median(v), max(v)) for k, v in got.items()}


def ms3(t):
    return [round(v * 1e3, 4) for v in t]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples-log2", type=int, default=26)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--lengths", default="1000,1920,4095,4096")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    for dname in args.dtypes.split(","):
        dtype = torch.float32 if dname == "f32" else torch.float64
        esize = 4 if dtype == torch.float32 else 8
        for ln in (int(v) for v in args.lengths.split(",")):
            d = Dft(ln, dev)
            m = d.conv_size
            rows = max(1, (1 << args.samples_log2) // ln)
            samples = rows * ln
            re = torch.randn((rows, ln), device=dev, dtype=dtype)
            im = torch.randn((rows, ln), device=dev, dtype=dtype)
            out = (torch.empty_like(re), torch.empty_like(im))
            z = torch.complex(re, im)
            d.forward(re, im, out=out)
            want = torch.fft.fft(z, dim=1)
            err = ((torch.complex(*out) - want).abs().amax(dim=1) / want.abs().amax(dim=1)).max().item()
            del want
            # the Hilbert yardstick: as many rows of N = 2M real samples, len = N - 2 (the general path), IMAG
            n = 2 * m
            plan = BatchedFft(n, dev, dtype)
            xh = torch.randn((rows, n), device=dev, dtype=dtype)[:, :n - 2]
            yh = torch.empty((rows, n), device=dev, dtype=dtype)
            t = timed_together({
                "dft": lambda: d.forward(re, im, out=out),
                "torch": lambda: torch.fft.fft(z, dim=1),
                "hilbert": lambda: plan.hilbert_imag(xh, out=yh),
            }, args.warmup, args.calls)
            t_k, t_h = t["dft"][1], t["hilbert"][1]
            tbps = samples * 4 * esize / t_k / 1e12
            rec = {"dtype": dname, "length": ln, "conv_size": m, "rows": rows, "samples": samples,
                   "dft_ms_min_med_max": ms3(t["dft"]), "dft_gsps": round(samples / t_k / 1e9, 3),
                   "dft_tbps": round(tbps, 3), "pct_of_8tbps": round(100 * tbps / PEAK_TBPS, 1),
                   "dft_mrows_per_s": round(rows / t_k / 1e6, 3),
                   "torch_ms_min_med_max": ms3(t["torch"]), "vs_torch": round(t["torch"][1] / t_k, 3),
                   "hilbert_n": n, "hilbert_general_imag_ms_min_med_max": ms3(t["hilbert"]),
                   "hilbert_mrows_per_s": round(rows / t_h / 1e6, 3), "vs_hilbert_per_row": round(t_h / t_k, 3),
                   "max_diff_vs_torch": float(f"{err:.3e}")}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del re, im, out, z, xh, yh, d
            plan.close()
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

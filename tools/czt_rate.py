#!/usr/bin/env python3
"""Rates of the chirp-z transform on the GPU: Czt.forward (one fused launch per call, pdsp_czt_kernel.h) against two
yardsticks timed in the same process:

  dft      Dft.forward at L' = M / 2, the longest length with the same M, on the same number of rows: the same two
           pass sets of M points, the same LDS and the same occupancy, so rows per second are expected close to 1.0 of
           it (bluestein_kernel moves 2 L' values in and out per row, czt_kernel L in and K out);
  torch    the same bins composed in torch: torch.fft.fft of the rows zero-padded to `pad` = 1 / step points, cut to
           the first K bins, where its output fits in --fft-bytes (default 16 GiB); else the complex matmul x @ W
           with W[n, k] = exp(-2 pi i n k / pad) built once outside the timing.  Outputs are compared.

(L, K, pad) = (1000, 1000, 4096), (4096, 256, 2^20), (4096, 4096, 16384), (1024, 3000, 8192), f32 and f64, 2^26 complex
input samples per call.  Device events; per function --warmup calls, then --calls timed calls, the functions alternating
call by call; min / median / max are recorded and the ratios use the medians.  Prints one JSON line per case: input
GSample/s, algorithmic TB/s (2 sizeof T (L + K) per row: what a call must move), rows per second of both kernels, and
the ratios.  Nothing here is a gate.

    python tools/czt_rate.py [--out profiles/czt_rate.jsonl] [--samples-log2 26]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pragma_dsp_amd.czt import Czt  # noqa: E402
from pragma_dsp_amd.dft import Dft  # noqa: E402

PEAK_TBPS = 8.0
CASES = [(1000, 1000, 4096), (4096, 256, 1 << 20), (4096, 4096, 16384), (1024, 3000, 8192)]


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
    ap.add_argument("--fft-bytes", type=int, default=16 << 30)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    for dname in args.dtypes.split(","):
        dtype = torch.float32 if dname == "f32" else torch.float64
        cdtype = torch.complex64 if dname == "f32" else torch.complex128
        esize = 4 if dtype == torch.float32 else 8
        for ln, bins, pad in CASES:
            c = Czt(ln, bins, 1.0 / pad, device=dev)
            m = c.conv_size
            rows = max(1, (1 << args.samples_log2) // ln)
            re = torch.randn((rows, ln), device=dev, dtype=dtype)
            im = torch.randn((rows, ln), device=dev, dtype=dtype)
            out = (torch.empty((rows, bins), device=dev, dtype=dtype), torch.empty((rows, bins), device=dev, dtype=dtype))
            z = torch.complex(re, im)
            if rows * pad * 2 * esize <= args.fft_bytes:
                how = "padded_fft"
                compose = lambda: torch.fft.fft(z, n=pad, dim=1)[:, :bins]  # noqa: E731
            else:
                how = "matmul"
                nk = (torch.arange(ln, device=dev, dtype=torch.int64)[:, None]
                      * torch.arange(bins, device=dev, dtype=torch.int64)[None, :]) % pad
                w = torch.polar(torch.ones((), device=dev, dtype=torch.float64),
                                nk.double() * (-2.0 * torch.pi / pad)).to(cdtype)
                del nk
                compose = lambda: z @ w  # noqa: E731
            c.forward(re, im, out=out)
            want = compose()
            err = ((torch.complex(*out) - want).abs().amax(dim=1) / want.abs().amax(dim=1)).max().item()
            del want
            # the DFT yardstick: as many rows of L' = M / 2 points
            ld = m // 2
            d = Dft(ld, dev)
            assert d.conv_size == m
            dre = torch.randn((rows, ld), device=dev, dtype=dtype)
            dim_ = torch.randn((rows, ld), device=dev, dtype=dtype)
            dout = (torch.empty_like(dre), torch.empty_like(dim_))
            t = timed_together({
                "czt": lambda: c.forward(re, im, out=out),
                "dft": lambda: d.forward(dre, dim_, out=dout),
                "torch": compose,
            }, args.warmup, args.calls)
            t_k, t_d = t["czt"][1], t["dft"][1]
            tbps = rows * (ln + bins) * 2 * esize / t_k / 1e12
            rec = {"dtype": dname, "length": ln, "bins": bins, "pad": pad, "conv_size": m, "rows": rows,
                   "samples": rows * ln,
                   "czt_ms_min_med_max": ms3(t["czt"]), "czt_gsps_in": round(rows * ln / t_k / 1e9, 3),
                   "czt_tbps": round(tbps, 3), "pct_of_8tbps": round(100 * tbps / PEAK_TBPS, 1),
                   "czt_mrows_per_s": round(rows / t_k / 1e6, 3),
                   "dft_length": ld, "dft_ms_min_med_max": ms3(t["dft"]),
                   "dft_mrows_per_s": round(rows / t_d / 1e6, 3), "vs_dft_per_row": round(t_d / t_k, 3),
                   "torch_how": how, "torch_ms_min_med_max": ms3(t["torch"]), "vs_torch": round(t["torch"][1] / t_k, 3),
                   "max_diff_vs_torch": float(f"{err:.3e}")}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del re, im, out, z, dre, dim_, dout, c, d, compose
            if how == "matmul":
                del w
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

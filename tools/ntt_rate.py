#!/usr/bin/env python3
"""Rates of the number-theoretic transform on the GPU: Ntt.forward / Ntt.inverse / Ntt.convolve (one fused launch per
call, pdsp_ntt_kernel.h) on 2^26 points per call at N = 1024, 4096 and 16384, each against yardsticks timed in the same
process, the functions alternating call by call:

  copy      torch's device copy of the same bytes (8 in + 8 out per point: the least a transform can move);
  fft_f64   BatchedFft's f64 complex rows of the same N (planar re / im, 16 bytes in + 16 out per point): the rows per
            second of the floating-point transform this one stands beside;
  composed  for CONV: forward(a), forward(b), ntt_mul, inverse -- the four launches the fused kernel replaces
            (64 bytes per point against its 24).

Before anything is timed the fused convolution is compared with the composition (equality of bits).  Device events; per
function --warmup calls, then --calls timed calls; min / median / max are recorded and the ratios use the medians.
Prints one JSON line per case.

    python tools/ntt_rate.py [--out profiles/ntt_rate.jsonl] [--points-log2 26]
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
from pragma_dsp_amd.ntt import Ntt, ntt_mul  # noqa: E402

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
    ap.add_argument("--points-log2", type=int, default=26)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--sizes-log2", default="10,12,14")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(20261019)
    lines = []
    for lg in (int(v) for v in args.sizes_log2.split(",")):
        n = 1 << lg
        rows = max(1, (1 << args.points_log2) >> lg)
        points = rows * n
        a = torch.randint(-(1 << 63), (1 << 63) - 1, (rows, n), device=dev, dtype=torch.int64, generator=gen)
        b = torch.randint(-(1 << 63), (1 << 63) - 1, (rows, n), device=dev, dtype=torch.int64, generator=gen)
        out, t1, t2 = torch.empty_like(a), torch.empty_like(a), torch.empty_like(a)
        plan = Ntt(n, dev)
        fft = BatchedFft(n, dev, torch.float64)
        re = torch.randn((rows, n), device=dev, dtype=torch.float64)
        im = torch.randn((rows, n), device=dev, dtype=torch.float64)
        fout = (torch.empty_like(re), torch.empty_like(im))

        def composed():
            plan.forward(a, out=t1)
            plan.forward(b, out=t2)
            ntt_mul(t1, t2, out=t1)
            return plan.inverse(t1, out=t2)

        same = bool(torch.equal(plan.convolve(a, b, out_len=n, out=out), composed()))
        back = plan.inverse(plan.forward(a))
        p = 0xFFFFFFFF00000001 - (1 << 64)  # p as the int64 of the same bits: patterns in [p, 2^64) are -2^32 + 1 ... -1
        roundtrip = bool(torch.equal(back, torch.where((a < 0) & (a >= p), a - p, a)))
        fns = {
            "forward": lambda: plan.forward(a, out=out),
            "inverse": lambda: plan.inverse(a, out=out),
            "conv": lambda: plan.convolve(a, b, out_len=n, out=out),
            "copy": lambda: out.copy_(a),
            "fft_f64": lambda: fft.forward(re, im, out=fout),
            "composed": composed,
        }
        t = timed_together(fns, args.warmup, args.calls)
        copy_tbps = points * 16 / t["copy"][1] / 1e12
        for op, bytes_per_point in (("forward", 16), ("inverse", 16), ("conv", 24)):
            t_k = t[op][1]
            tbps = points * bytes_per_point / t_k / 1e12
            rec = {"op": op, "n": n, "rows": rows, "points": points, "ms_min_med_max": ms3(t[op]),
                   "gpoints_per_s": round(points / t_k / 1e9, 3), "rows_per_s": round(rows / t_k, 1),
                   "bytes_per_point": bytes_per_point, "tbps": round(tbps, 3), "pct_of_8tbps": round(100 * tbps / PEAK_TBPS, 1),
                   "copy_ms_min_med_max": ms3(t["copy"]), "copy_tbps": round(copy_tbps, 3),
                   "time_over_copy": round(t_k / t["copy"][1], 3),
                   "fft_f64_ms_min_med_max": ms3(t["fft_f64"]), "fft_f64_rows_per_s": round(rows / t["fft_f64"][1], 1),
                   "fft_f64_tbps": round(points * 32 / t["fft_f64"][1] / 1e12, 3),
                   "time_over_fft_f64": round(t_k / t["fft_f64"][1], 3)}
            if op == "conv":
                rec.update({"composed_ms_min_med_max": ms3(t["composed"]), "composed_over_fused": round(t["composed"][1] / t_k, 3),
                            "fused_equals_composed": same})
            else:
                rec["roundtrip_exact"] = roundtrip
            print(json.dumps(rec), flush=True)
            lines.append(rec)
        del a, b, out, t1, t2, re, im, fout, plan, fft
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

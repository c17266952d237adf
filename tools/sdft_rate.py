#!/usr/bin/env python3
"""Rates of the sliding DFT on the GPU: SlidingDft.forward (one launch per call, pdsp_sdft_kernel.h) on 2^26 input
samples per call (64 rows of 2^20) at N = 1024, 4096 and 1000, K = 1, 8 and 32 bins, hop 1, 16 and N / 4, rectangular
and Hann, f32 and f64 -- each against yardsticks timed in the same process, the functions alternating call by call:

  copy      torch's device copy of the same bytes (the input read once and 2 K F values written: at hop 1 the output is
            2 K times the input, so the copy is the yardstick);
  stft      BatchedFft.stft_complex of the same samples at the same (N, hop) plus the gather of the K bins, where N is
            a power of two and its output ((N + 2) / hop values per sample) fits in --max-gib;
  torch     unfold + two real matmuls with the K x N cosine and sine matrices (the window folded in), where the
            frames torch materialises fit in --max-gib.

Before anything is timed the kernel's bins are compared with the torch composition's where that runs.  Device events;
per function --warmup calls, then --calls timed calls; min / median / max are recorded and the ratios use the medians.
Prints one JSON line per case.

    python tools/sdft_rate.py [--out profiles/sdft_rate.jsonl] [--sizes 1024,4096,1000] [--ks 1,8,32] [--dtypes f32,f64]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pragma_dsp_amd import createWindow  # noqa: E402
from pragma_dsp_amd.batch import BatchedFft  # noqa: E402
from pragma_dsp_amd.sdft import SlidingDft  # noqa: E402

PEAK_TBPS = 8.0
DT = {"f32": torch.float32, "f64": torch.float64}


def timed_together(fns, warmup, calls):
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
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--row-log2", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--sizes", default="1024,4096,1000")
    ap.add_argument("--ks", default="1,8,32")
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--windows", default="rect,hann")
    ap.add_argument("--max-gib", type=float, default=24.0)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rows, t = args.rows, 1 << args.row_log2
    cap = args.max_gib * 2 ** 30
    lines = []
    for dname in args.dtypes.split(","):
        dt = DT[dname]
        eb = 4 if dname == "f32" else 8
        x = torch.randn((rows, t), device=dev, dtype=dt)
        for n in (int(v) for v in args.sizes.split(",")):
            pow2 = n & (n - 1) == 0
            for k in (int(v) for v in args.ks.split(",")):
                bins = [float(1 + (j * (n // 2 - 1)) // max(1, k - 1)) for j in range(k)]  # integers in 1 ... N / 2
                for h in (1, 16, n // 4):
                    for win in args.windows.split(","):
                        s = SlidingDft(n, bins, hop=h, window=win, device=dev)
                        f = s.frames(t)
                        out = (torch.empty((rows, k, f), device=dev, dtype=dt), torch.empty((rows, k, f), device=dev, dtype=dt))
                        in_b, out_b = rows * t * eb, 2 * rows * k * f * eb
                        half = (in_b + out_b) // (2 * eb)
                        src, dst = torch.empty(half, device=dev, dtype=dt), torch.empty(half, device=dev, dtype=dt)
                        fns = {"sdft": lambda: s.forward(x, out=out), "copy": lambda: dst.copy_(src)}
                        # stft_complex of the same samples as one signal, then the K bins
                        frames_all = 1 + (rows * t - n) // h
                        stft_b = 2 * frames_all * (n // 2 + 1) * eb
                        if pow2 and stft_b <= cap:
                            plan = BatchedFft(n, dev, dt)
                            idx = torch.tensor([int(b) for b in bins], device=dev)
                            flat = x.reshape(-1)

                            def stft():
                                re, im = plan.stft_complex(flat, h, win)
                                return re.index_select(1, idx), im.index_select(1, idx)
                            fns["stft"] = stft
                        # unfold + matmul: torch copies the overlapping frames
                        agree = None
                        if rows * f * n * eb <= cap:
                            w = np.asarray(createWindow(win, n), dtype=np.float64)
                            ang = -2 * np.pi * np.outer(np.arange(n), np.asarray(bins)) / n
                            cm = torch.from_numpy(w[:, None] * np.cos(ang)).to(dt).to(dev)
                            sm = torch.from_numpy(w[:, None] * np.sin(ang)).to(dt).to(dev)

                            def composed():
                                fr = x.unfold(1, n, h)  # [rows, F, N]
                                return torch.matmul(fr, cm), torch.matmul(fr, sm)
                            fns["torch"] = composed
                            cr, ci = composed()
                            got = s.forward(x, out=out)
                            scale = float(cr.abs().max())
                            agree = max(float((got[0].transpose(1, 2) - cr).abs().max()),
                                        float((got[1].transpose(1, 2) - ci).abs().max())) / scale
                            del cr, ci
                        tm = timed_together(fns, args.warmup, args.calls)
                        t_k = tm["sdft"][1]
                        rec = {"dtype": dname, "n": n, "k": k, "hop": h, "window": win, "components": s.components,
                               "rows": rows, "samples_per_row": t, "frames": f, "ms_min_med_max": ms3(tm["sdft"]),
                               "gsamples_in_per_s": round(rows * t / t_k / 1e9, 3),
                               "gbin_samples_per_s": round(rows * t * k / t_k / 1e9, 3),
                               "algorithmic_tbps": round((in_b + out_b) / t_k / 1e12, 4),
                               "pct_of_8tbps": round(100 * (in_b + out_b) / t_k / 1e12 / PEAK_TBPS, 2),
                               "copy_ms_min_med_max": ms3(tm["copy"]),
                               "copy_tbps": round((in_b + out_b) / tm["copy"][1] / 1e12, 3),
                               "time_over_copy": round(t_k / tm["copy"][1], 2),
                               "stft_ms_min_med_max": ms3(tm["stft"]) if "stft" in tm else None,
                               "stft_over_sdft": round(tm["stft"][1] / t_k, 3) if "stft" in tm else None,
                               "torch_ms_min_med_max": ms3(tm["torch"]) if "torch" in tm else None,
                               "torch_over_sdft": round(tm["torch"][1] / t_k, 3) if "torch" in tm else None,
                               "max_diff_to_torch_over_max": agree}
                        print(json.dumps(rec), flush=True)
                        lines.append(rec)
                        del s, out, src, dst, fns
                        torch.cuda.empty_cache()
        del x
    if args.out:
        with open(args.out, "w") as fh:
            for r in lines:
                fh.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

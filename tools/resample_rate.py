#!/usr/bin/env python3
"""Rates of the polyphase rate-change kernel on the GPU: Resampler.apply (one time-domain launch per call,
pdsp_upfirdn_kernel.h) against two yardsticks timed in the same process on the same inputs, outputs compared:
(a) the torch composition -- a zero-stuffed copy, then torch.nn.functional.conv1d with stride=down -- and (b) for
up = 1 what a user of this library did before: FirFilter.apply(mode="full") followed by a strided slice.  f32 and
f64, about 2^26 input samples per call in rows of 2^16 (and one case of 2^12), default taps, ratios 2/1, 1/2, 4/1,
1/8, 3/2, 160/147 and 147/160.  The torch composition runs on the first rows only, as many as keep its stuffed copy
at --torch-log2 samples, and its time is scaled to the whole batch by rows.  Device events; per function 5 warm-up
calls, then --windows windows of about --window-s seconds each, the functions alternating window by window; min /
median / max of the windows are recorded and the ratios use the medians.  Prints one JSON line per case: GSample/s of
max(in, out), algorithmic TB/s (len in plus y_len out per row: what a call must move), its share of 8 TB/s, and the
two ratios (yardstick time / kernel time: above 1 the kernel is faster).

    python tools/resample_rate.py [--out profiles/resample_rate.jsonl] [--samples-log2 26] [--window-s 0.15]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from hilbert_rate import ms3, timed_together  # noqa: E402
from pragma_dsp_amd.filters import FirFilter  # noqa: E402
from pragma_dsp_amd.resample import Resampler  # noqa: E402

PEAK_TBPS = 8.0
RATIOS = ((2, 1), (1, 2), (4, 1), (1, 8), (3, 2), (160, 147), (147, 160))


def torch_resample(x, r, taps_flipped, y_len):
    """Zero-stuff, pad so that output m reads taps m down + t0 - i, conv1d with stride down."""
    rows, n = x.shape
    left = r.ntaps - 1 - r.t0
    total = (y_len - 1) * r.down + r.ntaps
    z = torch.zeros((rows, 1, max(total, left + (n - 1) * r.up + 1)), dtype=x.dtype, device=x.device)
    z[:, 0, left:left + (n - 1) * r.up + 1:r.up] = x
    return torch.nn.functional.conv1d(z[:, :, :total], taps_flipped, stride=r.down)[:, 0, :y_len]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples-log2", type=int, default=26)
    ap.add_argument("--torch-log2", type=int, default=24)
    ap.add_argument("--window-s", type=float, default=0.15)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--dtypes", default="f32,f64")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    cases = [(u, d, 1 << 16) for u, d in RATIOS] + [(3, 2, 1 << 12)]
    for dname in args.dtypes.split(","):
        dtype = torch.float32 if dname == "f32" else torch.float64
        esize = 4 if dtype == torch.float32 else 8
        for up, down, n in cases:
            r = Resampler(up, down, device=dev, dtype=dtype)
            rows = (1 << args.samples_log2) // n
            y_len = r.output_len(n)
            x = torch.randn((rows, n), device=dev, dtype=dtype)
            y = torch.empty((rows, y_len), device=dev, dtype=dtype)
            r.apply(x, out=y)
            scale = (x.abs().amax() * float(abs(r.taps).sum())).item()
            fns = {"kernel": lambda: r.apply(x, out=y)}
            rec = {"dtype": dname, "up": up, "down": down, "len": n, "rows": rows, "ntaps": r.ntaps}
            # (a) torch, on the first rows
            trows = max(1, min(rows, (1 << args.torch_log2) // (n * up)))
            w = torch.from_numpy(r.taps[::-1].copy()).to(dtype).to(dev).view(1, 1, -1)
            try:
                got = torch_resample(x[:trows], r, w, y_len)
                rec["max_diff_vs_torch"] = float(f"{((got - y[:trows]).abs().max().item() / scale):.3e}")
                del got
                fns["torch"] = lambda: torch_resample(x[:trows], r, w, y_len)
            except RuntimeError as exc:  # a convolution torch does not have in this precision
                rec["torch_error"] = str(exc).splitlines()[0][:120]
            # (b) FirFilter full + slice (up = 1)
            if up == 1:
                fir = FirFilter(r.taps, dev, dtype)
                full = torch.empty((rows, n + r.ntaps - 1), device=dev, dtype=dtype)

                def fir_way():
                    fir.apply(x, "full", out=full)
                    return full[:, r.t0::down][:, :y_len].contiguous()
                got = fir_way()
                rec["max_diff_vs_fir"] = float(f"{((got - y).abs().max().item() / scale):.3e}")
                del got
                fns["fir"] = fir_way
            t = timed_together(fns, args.window_s, args.windows)
            t_k = t["kernel"][1]
            moved = rows * (n + y_len) * esize
            tbps = moved / t_k / 1e12
            rec.update({"kernel_ms_min_med_max": ms3(t["kernel"]),
                        "gsps": round(rows * max(n, y_len) / t_k / 1e9, 2), "tbps": round(tbps, 3),
                        "pct_of_8tbps": round(100 * tbps / PEAK_TBPS, 1)})
            if "torch" in t:
                tt = tuple(v * rows / trows for v in t["torch"])
                rec.update({"torch_rows": trows, "torch_ms_min_med_max_scaled": ms3(tt), "vs_torch": round(tt[1] / t_k, 2)})
            if "fir" in t:
                rec.update({"fir_ms_min_med_max": ms3(t["fir"]), "vs_fir": round(t["fir"][1] / t_k, 2)})
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del x, y, fns
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Rates of the 2-D transform on the GPU: Fft2d.forward (pdsp_fft2d_kernel.h: one resident launch up to 4096 points
per image, else the row kernels and one column launch) against three yardsticks timed in the same process:

  composed  the library's own public calls as they were before the 2-D transform existed: BatchedFft(W).forward on the
            rows, a torch transpose to contiguous, BatchedFft(H).forward, and the transpose back (outputs compared);
  torch     torch's own 2-D FFT on the same images as one complex tensor (rocFFT; outputs compared);
  copy      the device copy of the same bytes (both planes in, both planes out).

and, for the resident 64 x 64 f32 case, the N = 4096 C2C row kernel on the same number of samples (the same LDS
footprint and HBM traffic per sample).

Shapes: 2^26 samples per call at 64 x 64, 16 x 256, 64 x 256, 128 x 1024, 512 x 512 and 256 x 4096, f32 and f64,
forward, complex in and out.  Device events; per function --warmup calls, then --calls timed calls, the functions
alternating call by call; min / median / max are recorded and the ratios use the medians.  Algorithmic bytes come from
the shapes: 4 sizeof T per sample (16 B in f32, 32 B in f64) for complex in and out; a real input would be 3 sizeof T.
Prints one JSON line per case.

    python tools/fft2d_rate.py [--out profiles/fft2d_rate.jsonl] [--samples-log2 26]
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
from pragma_dsp_amd.fft2d import Fft2d  # noqa: E402

PEAK_TBPS = 8.0
SHAPES = "64x64,16x256,64x256,128x1024,512x512,256x4096"


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
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--shapes", default=SHAPES)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    for dname in args.dtypes.split(","):
        dtype = torch.float32 if dname == "f32" else torch.float64
        esize = 4 if dtype == torch.float32 else 8
        for h, w in (tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")):
            f = Fft2d(h, w, dev)
            q = f.query(dtype)
            batch = max(1, (1 << args.samples_log2) // (h * w))
            samples = batch * h * w
            re = torch.randn((batch, h, w), device=dev, dtype=dtype)
            im = torch.randn((batch, h, w), device=dev, dtype=dtype)
            out = (torch.empty_like(re), torch.empty_like(im))
            cre, cim = torch.empty_like(re), torch.empty_like(im)
            rows_w, rows_h = BatchedFft(w, dev, dtype), BatchedFft(h, dev, dtype)
            r1, i1 = torch.empty((batch * h, w), device=dev, dtype=dtype), torch.empty((batch * h, w), device=dev, dtype=dtype)
            r2, i2 = torch.empty((batch * w, h), device=dev, dtype=dtype), torch.empty((batch * w, h), device=dev, dtype=dtype)

            def composed():
                rows_w.forward(re.view(batch * h, w), im.view(batch * h, w), out=(r1, i1))
                tr = r1.view(batch, h, w).transpose(1, 2).contiguous()
                ti = i1.view(batch, h, w).transpose(1, 2).contiguous()
                rows_h.forward(tr.view(batch * w, h), ti.view(batch * w, h), out=(r2, i2))
                return (r2.view(batch, w, h).transpose(1, 2).contiguous(), i2.view(batch, w, h).transpose(1, 2).contiguous())

            def copy():
                cre.copy_(re)
                cim.copy_(im)

            z = torch.complex(re, im)
            f.forward(re, im, out=out)
            want = torch.fft.fft2(z)
            scale = want.abs().amax(dim=(1, 2))
            err_torch = ((torch.complex(*out) - want).abs().amax(dim=(1, 2)) / scale).max().item()
            comp = composed()
            err_comp = ((torch.complex(*out) - torch.complex(*comp)).abs().amax(dim=(1, 2)) / scale).max().item()
            del want, comp, scale
            fns = {"fft2d": lambda: f.forward(re, im, out=out), "composed": composed,
                   "torch": lambda: torch.fft.fft2(z), "copy": copy}
            rows4096 = None
            if (h, w) == (64, 64) and dname == "f32":
                rows4096 = BatchedFft(4096, dev, dtype)
                fns["rows4096"] = lambda: rows4096.forward(re.view(-1, 4096), im.view(-1, 4096), out=(r1.view(-1, 4096), i1.view(-1, 4096)))
            t = timed_together(fns, args.warmup, args.calls)
            t_k = t["fft2d"][1]
            tbps = samples * 4 * esize / t_k / 1e12
            rec = {"dtype": dname, "height": h, "width": w, "batch": batch, "samples": samples, "path": q["path"],
                   "images_per_workgroup": q["images_per_workgroup"], "tile": q["tile"],
                   "bytes_per_sample": 4 * esize, "bytes_per_sample_real_in": 3 * esize,
                   "fft2d_ms_min_med_max": ms3(t["fft2d"]), "fft2d_gsps": round(samples / t_k / 1e9, 3),
                   "fft2d_tbps": round(tbps, 3), "pct_of_8tbps": round(100 * tbps / PEAK_TBPS, 1),
                   "composed_ms_min_med_max": ms3(t["composed"]), "vs_composed": round(t["composed"][1] / t_k, 3),
                   "torch_ms_min_med_max": ms3(t["torch"]), "vs_torch": round(t["torch"][1] / t_k, 3),
                   "copy_ms_min_med_max": ms3(t["copy"]), "vs_copy": round(t["copy"][1] / t_k, 3),
                   "max_diff_vs_torch": float(f"{err_torch:.3e}"), "max_diff_vs_composed": float(f"{err_comp:.3e}")}
            if rows4096 is not None:
                rec["rows4096_ms_min_med_max"] = ms3(t["rows4096"])
                rec["vs_rows4096"] = round(t["rows4096"][1] / t_k, 3)
                rows4096.close()
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            del re, im, out, cre, cim, r1, i1, r2, i2, z, f
            rows_w.close()
            rows_h.close()
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fo:
            for r in lines:
                fo.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

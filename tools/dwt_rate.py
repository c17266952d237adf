#!/usr/bin/env python3
"""Rates of the multi-level wavelet transform on the GPU: Dwt.forward / Dwt.inverse (one fused launch per call,
pdsp_dwt_kernel.h) against the same result composed two ways, timed in the same process:

  torch    one torch.nn.functional.conv1d per level (both filters as two output channels, stride 2) on the row
           extended periodically by F - 2 samples; the inverse one conv_transpose1d per level whose F - 2 trailing
           outputs are folded back onto the head;
  upfirdn  what this library offered before: Upfirdn(reversed h, 1, 2) and Upfirdn(reversed g, 1, 2) per level on
           the extended row (the inverse: Upfirdn(h, 2, 1) + Upfirdn(g, 2, 1) and the fold), the extension, the slices
           and the sums made in torch.

Both compositions are compared with the kernel's output before anything is timed.  Rows of 4096 (the resident path)
and of 2^16 and 2^20 (tiled), db2 and db8, J = 1, 4, 8, forward and inverse, f32 and f64, 2^26 samples per call.
Device events; per function --warmup calls, then --calls timed calls, the functions alternating call by call; min /
median / max are recorded and the ratios use the medians.  Prints one JSON line per case: GSample/s, algorithmic TB/s
(sizeof T in plus sizeof T out per sample: what a call must move, whatever J is), its share of 8 TB/s, and the time of
each composition over ours.

    python tools/dwt_rate.py [--out profiles/dwt_rate.jsonl] [--samples-log2 26]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from pragma_dsp_amd._capi import check, lib  # noqa: E402
from pragma_dsp_amd.resample import Upfirdn  # noqa: E402
from pragma_dsp_amd.wavelet import Dwt  # noqa: E402

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


def extend(a, extra):
    """a [rows, m] followed by its first `extra` samples, periodically (extra may exceed m)."""
    m = a.shape[-1]
    reps = -(-(m + extra) // m)
    return a.repeat(1, reps)[:, :m + extra] if reps > 2 else torch.cat([a, a[:, :extra]], dim=1)


def fold(y, m):
    """y [rows, m + tail] -> [rows, m]: the tail wraps onto the head, periodically."""
    out = y[:, :m].clone()
    pos = m
    while pos < y.shape[1]:
        k = min(m, y.shape[1] - pos)
        out[:, :k] += y[:, pos:pos + k]
        pos += k
    return out


class TorchComposition:
    def __init__(self, h, g, levels, dtype, dev):
        self.levels, self.f = levels, h.numel()
        self.w = torch.stack([h, g]).to(dtype).to(dev).reshape(2, 1, -1)

    def forward(self, x):
        a, bands = x, []
        for _ in range(self.levels):
            y = F.conv1d(extend(a, self.f - 2).unsqueeze(1), self.w, stride=2)
            a = y[:, 0]
            bands.append(y[:, 1])
        return torch.cat([a] + bands[::-1], dim=1)

    def inverse(self, c):
        m = c.shape[1] >> self.levels
        a = c[:, :m]
        for _ in range(self.levels):
            y = F.conv_transpose1d(torch.stack([a, c[:, m:2 * m]], dim=1), self.w, stride=2)[:, 0]
            m *= 2
            a = fold(y, m)
        return a


class UpfirdnComposition:
    def __init__(self, h, g, levels, dtype, dev):
        self.levels, self.f = levels, h.numel()
        self.dec = [Upfirdn(t.flip(0), 1, 2, dev, dtype) for t in (h, g)]
        self.itp = [Upfirdn(t, 2, 1, dev, dtype) for t in (h, g)]

    def forward(self, x):
        a, bands, s = x, [], self.f // 2
        for _ in range(self.levels):
            m = a.shape[1]
            e = torch.cat([a[:, -1:], extend(a, self.f - 2)], dim=1)  # one sample in front: F - 1 is odd
            lo, hi = (u.apply(e)[:, s:s + m // 2] for u in self.dec)
            a = lo
            bands.append(hi)
        return torch.cat([a] + bands[::-1], dim=1)

    def inverse(self, c):
        m = c.shape[1] >> self.levels
        a = c[:, :m]
        for _ in range(self.levels):
            y = self.itp[0].apply(a.contiguous()) + self.itp[1].apply(c[:, m:2 * m].contiguous())
            m *= 2
            a = fold(y, m)
        return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples-log2", type=int, default=26)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--dtypes", default="f32,f64")
    ap.add_argument("--rows-log2", default="12,16,20")
    ap.add_argument("--wavelets", default="db2,db8")
    ap.add_argument("--levels", default="1,4,8")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    for dname in args.dtypes.split(","):
        dtype = torch.float32 if dname == "f32" else torch.float64
        esize = 4 if dtype == torch.float32 else 8
        for lg in (int(v) for v in args.rows_log2.split(",")):
            n = 1 << lg
            rows = max(1, (1 << args.samples_log2) >> lg)
            samples = rows * n
            x = torch.randn((rows, n), device=dev, dtype=dtype)
            out = torch.empty_like(x)
            for name in args.wavelets.split(","):
                for levels in (int(v) for v in args.levels.split(",")):
                    w = Dwt(name, levels, dev, dtype)
                    h = torch.from_numpy(w.taps)
                    g = h.flip(0) * torch.tensor([(-1.0) ** j for j in range(h.numel())], dtype=h.dtype)
                    comps = {"torch": TorchComposition(h, g, levels, dtype, dev),
                             "upfirdn": UpfirdnComposition(h, g, levels, dtype, dev)}
                    for direction in ("forward", "inverse"):
                        info = (C.c_longlong * 5)()
                        check(lib.pdsp_dev_dwt_tile(w.ntaps, levels, n, esize, int(direction == "inverse"), info))
                        path = "resident" if info[0] else f"tiled, T = {info[1]}"
                        run = getattr(w, direction)
                        run(x, out=out)
                        scale = out.abs().max().item()
                        diff = {k: (getattr(c, direction)(x) - out).abs().max().item() / scale for k, c in comps.items()}
                        fns = {"dwt": lambda: run(x, out=out)}
                        fns.update({k: (lambda c=c: getattr(c, direction)(x)) for k, c in comps.items()})
                        t = timed_together(fns, args.warmup, args.calls)
                        t_k = t["dwt"][1]
                        tbps = samples * 2 * esize / t_k / 1e12
                        rec = {"dtype": dname, "row": n, "rows": rows, "samples": samples, "wavelet": name,
                               "taps": int(h.numel()), "levels": levels, "direction": direction, "path": path,
                               "dwt_ms_min_med_max": ms3(t["dwt"]), "dwt_gsps": round(samples / t_k / 1e9, 3),
                               "dwt_tbps": round(tbps, 3), "pct_of_8tbps": round(100 * tbps / PEAK_TBPS, 1),
                               "torch_ms_min_med_max": ms3(t["torch"]), "vs_torch": round(t["torch"][1] / t_k, 3),
                               "upfirdn_ms_min_med_max": ms3(t["upfirdn"]), "vs_upfirdn": round(t["upfirdn"][1] / t_k, 3),
                               "max_diff_vs_torch": float(f"{diff['torch']:.3e}"),
                               "max_diff_vs_upfirdn": float(f"{diff['upfirdn']:.3e}")}
                        print(json.dumps(rec), flush=True)
                        lines.append(rec)
                    del w, comps
                    torch.cuda.empty_cache()
            del x, out
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

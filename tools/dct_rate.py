#!/usr/bin/env python3
"""Rates of the DCT on the GPU: BatchedFft.dct of types 2 and 3 (one fused launch per call, pdsp_dct_kernel.h)
against the same DCT composed in torch (a gather for the permutation, torch.fft.rfft / irfft, the twiddle multiply;
same card, same process, same inputs, outputs compared), f32 and f64, N = 1024 / 4096 / 16384, 2^26 samples per
call, norm "backward".  Device events, 2 warm-up calls, then the mean of --iters timed calls.  Prints one JSON line
per case: GSample/s, algorithmic TB/s (2 N sizeof T per row: what a call must move, not what it moves) and its share
of 8 TB/s.

    python tools/dct_rate.py [--out profiles/dct_rate.jsonl] [--samples-log2 26] [--iters 20]
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pragma_dsp_amd.batch import BatchedFft  # noqa: E402

PEAK_TBPS = 8.0


def timed(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


class TorchDct:
    """scipy.fft.dct(x, type) with norm "backward" by Makhoul's algorithm in torch ops."""

    def __init__(self, n, dev, dtype):
        m = n // 2
        self.n, self.m = n, m
        idx = torch.arange(n, device=dev)
        self.perm = torch.cat([idx[0::2], idx[1::2].flip(0)])  # v = x[perm]
        self.unperm = torch.empty_like(self.perm)
        self.unperm[self.perm] = idx  # y = v[unperm]
        k = torch.arange(m + 1, device=dev, dtype=torch.float64)
        cdt = torch.complex64 if dtype == torch.float32 else torch.complex128
        self.w4 = torch.exp(-1j * math.pi * k / (2 * n)).to(cdt)
        self.rev = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), torch.arange(n - 1, m - 1, -1, device=dev)])

    def dct2(self, x):
        c = self.w4 * torch.fft.rfft(x[:, self.perm], dim=1)
        return torch.cat([2 * c.real, (-2 * c.imag[:, 1:self.m]).flip(1)], dim=1)

    def dct3(self, x):
        xr = x[:, self.rev]  # x[N - k], k = 0 ... M (k = 0 zeroed below)
        xr[:, 0] = 0
        v = torch.fft.irfft(self.w4.conj() * torch.complex(x[:, :self.m + 1], -xr), n=self.n, dim=1) * self.n
        return v[:, self.unperm]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples-log2", type=int, default=26)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    for dtype in (torch.float32, torch.float64):
        esize = 4 if dtype == torch.float32 else 8
        for n in (1024, 4096, 16384):
            plan = BatchedFft(n, dev, dtype)
            ref = TorchDct(n, dev, dtype)
            rows = (1 << args.samples_log2) // n
            x = torch.randn((rows, n), device=dev, dtype=dtype)
            y = torch.empty_like(x)
            for t in (2, 3):
                tfn = ref.dct2 if t == 2 else ref.dct3
                plan.dct(x, type=t, out=y)
                want = tfn(x)
                err = ((y - want).abs().amax(dim=1) / want.abs().amax(dim=1)).max().item()
                del want
                t_k = timed(lambda: plan.dct(x, type=t, out=y), args.iters)
                t_t = timed(lambda: tfn(x), args.iters)
                samples = rows * n
                tbps = 2 * samples * esize / t_k / 1e12
                rec = {"dtype": "f32" if esize == 4 else "f64", "n": n, "type": t, "rows": rows, "samples": samples,
                       "dct_ms": round(t_k * 1e3, 4), "dct_gsps": round(samples / t_k / 1e9, 2),
                       "dct_tbps": round(tbps, 3), "pct_of_8tbps": round(100 * tbps / PEAK_TBPS, 1),
                       "torch_ms": round(t_t * 1e3, 4), "vs_torch": round(t_t / t_k, 2),
                       "max_rel_diff_vs_torch": float(f"{err:.3e}")}
                print(json.dumps(rec), flush=True)
                lines.append(rec)
            del x, y
            torch.cuda.empty_cache()
            plan.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

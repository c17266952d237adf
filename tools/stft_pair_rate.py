#!/usr/bin/env python3
"""Rates of the short-time pair on the GPU: BatchedFft.stft_complex and BatchedFft.istft against torch.stft /
torch.istft (center=False, the same Hamming window -- torch.istft refuses the symmetric Hann at hop = N --, same card,
same process), f32 and f64, N = 1024 / 4096 / 16384,
hop = N, N/2, N/4, at least 2^26 output samples per call.  Prints one JSON line per case:
GSample/s of signal, algorithmic TB/s (stft: signal in + bins out; istft: bins in + samples out -- what a call must
move, not what it moves), and the stream-ordered scratch the two-pass inverse adds (pdsp_istft_*: hop < N).

    python tools/stft_pair_rate.py [--out profiles/stft_pair_rate.jsonl] [--samples-log2 26]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from pragma_dsp_amd.batch import BatchedFft  # noqa: E402


def timed(fn, iters=5):
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


def scratch_bytes(n, hop, frames, esize):
    """The bound of pdsp_istft_* (include/pdsp_hip.h): min(S + K, frames) rows of N values."""
    if hop >= n:
        return 0
    k = -(-n // hop) - 1
    s = max(k + 1, (1 << 28) // (n * esize) - k)
    return min(s + k, frames) * n * esize


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples-log2", type=int, default=26)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lines = []
    for dtype in (torch.float32, torch.float64):
        esize = 4 if dtype == torch.float32 else 8
        for n in (1024, 4096, 16384):
            plan = BatchedFft(n, dev, dtype)
            w = plan.window("hamming").tensor()  # torch.istft refuses the symmetric Hann at hop = N (NOLA)
            for hop in (n, n // 2, n // 4):
                frames = ((1 << args.samples_log2) - n) // hop + 1
                total = (frames - 1) * hop + n
                bins = n // 2 + 1
                x = torch.randn(total, device=dev, dtype=dtype)
                re, im = plan.stft_complex(x, hop, "hamming")
                out = torch.empty(total, device=dev, dtype=dtype)
                t_f = timed(lambda: plan.stft_complex(x, hop, "hamming"))
                t_i = timed(lambda: plan.istft(re, im, hop, "hamming", out=out))
                spec = torch.stft(x, n_fft=n, hop_length=hop, window=w, center=False, return_complex=True)
                t_tf = timed(lambda: torch.stft(x, n_fft=n, hop_length=hop, window=w, center=False, return_complex=True))
                t_ti = timed(lambda: torch.istft(spec, n_fft=n, hop_length=hop, window=w, center=False, length=total))
                fwd_bytes = esize * (total + 2 * frames * bins)
                inv_bytes = esize * (2 * frames * bins + total)
                rec = {"dtype": "f32" if esize == 4 else "f64", "n": n, "hop": hop, "frames": frames, "samples": total,
                       "stft_ms": round(t_f * 1e3, 4), "stft_gsps": round(total / t_f / 1e9, 2),
                       "stft_tbps": round(fwd_bytes / t_f / 1e12, 3),
                       "istft_ms": round(t_i * 1e3, 4), "istft_gsps": round(total / t_i / 1e9, 2),
                       "istft_tbps": round(inv_bytes / t_i / 1e12, 3),
                       "torch_stft_ms": round(t_tf * 1e3, 4), "torch_istft_ms": round(t_ti * 1e3, 4),
                       "stft_vs_torch": round(t_tf / t_f, 2), "istft_vs_torch": round(t_ti / t_i, 2),
                       "istft_scratch_bytes": scratch_bytes(n, hop, frames, esize)}
                print(json.dumps(rec), flush=True)
                lines.append(rec)
                del x, re, im, out, spec
                torch.cuda.empty_cache()
            plan.close()
    if args.out:
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()

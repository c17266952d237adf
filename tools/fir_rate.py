#!/usr/bin/env python3
"""FIR filtering rate on the GPU box: the fused overlap-save kernel (FirFilter.apply) against the same filtering
composed from the existing launches and against torch.fft overlap-save (an outside reference point, never on the
product path).  Per N in {1024, 4096, 16384}, P in {N/16, N/4, N/2}, f32 and f64, mode "filter" on `rows` rows of
`len` samples:
  fused     FirFilter(taps, block=N).apply(x, "filter")                 one launch
  composed  materialised frames (torch gather) -> pdsp_fft_forward_real -> pdsp_complex_op_f32 MUL (f64: torch's
            complex multiply: the engine has no f64 complex_op) -> pdsp_fft_inverse -> copy of the valid samples
  torch     unfold -> torch.fft.rfft -> * H -> torch.fft.irfft -> slice
GSample/s counts output samples; "alg TB/s" counts the fused kernel's algorithmic bytes, len * N / hop reads +
y_len writes (the other two move far more).  Prints one line per case and a JSON line per case when --json.

    python tools/fir_rate.py [--rows 32] [--len 1048576] [--iters 10] [--json out.jsonl]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import pragma_dsp_amd as pd  # noqa: E402
from pragma_dsp_amd.batch import BatchedFft, complex_mul  # noqa: E402

dev = torch.device("cuda", 0)


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e-3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=32)
    ap.add_argument("--len", type=int, default=1 << 20)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    out = open(a.json, "a") if a.json else None
    rng = np.random.default_rng(0)
    for dtype in (torch.float32, torch.float64):
        esz = 4 if dtype == torch.float32 else 8
        x = torch.from_numpy(rng.standard_normal((a.rows, a.len))).to(dtype).to(dev)
        for n in (1024, 4096, 16384):
            plan = BatchedFft(n, dev, dtype)
            for p in (n // 16, n // 4, n // 2):
                h = rng.standard_normal(p)
                f = pd.FirFilter(h, dev, dtype, block=n)
                y = torch.empty(a.rows, a.len, dtype=dtype, device=dev)
                t_fused = timed(lambda: f.apply(x, "filter", out=y), a.iters)
                pk = p | 1  # the fused kernel's taps (one zero tap on an even filter)
                hop = n - pk + 1
                nblk = -(-a.len // hop)
                alg = esz * (a.rows * a.len * n / hop + a.rows * a.len)
                # composed: frames [rows * nblk, N] of the zero-padded signal (block b starts at b*hop - (P-1))
                xp = torch.nn.functional.pad(x, (pk - 1, nblk * hop + n - a.len))
                idx = (torch.arange(nblk, device=dev)[:, None] * hop + torch.arange(n, device=dev)[None, :]).reshape(-1)
                hf = torch.from_numpy(np.fft.fft(h, n)).to(dev)
                hre, him = hf.real.to(dtype).contiguous(), hf.imag.to(dtype).contiguous()

                def composed():
                    frames = xp[:, idx].reshape(-1, n)
                    xr, xi = plan.forward(frames)
                    if dtype == torch.float32:
                        yr, yi = complex_mul((xr, xi), (hre, him))
                    else:
                        z = torch.complex(xr, xi) * torch.complex(hre, him)
                        yr, yi = z.real.contiguous(), z.imag.contiguous()
                    tr, _ = plan.inverse(yr, yi)
                    return tr.reshape(a.rows, nblk, n)[:, :, pk - 1:].reshape(a.rows, -1)[:, :a.len].contiguous()

                t_comp = timed(composed, max(2, a.iters // 2))
                hr = torch.fft.rfft(torch.from_numpy(h).to(dtype).to(dev), n)

                def torch_os():
                    frames = xp.unfold(1, n, hop)[:, :nblk]
                    yb = torch.fft.irfft(torch.fft.rfft(frames, n) * hr, n)
                    return yb[..., pk - 1:].reshape(a.rows, -1)[:, :a.len]

                t_torch = timed(torch_os, max(2, a.iters // 2))
                # spot check: the three agree
                yc = composed()
                yt = torch_os()
                torch.cuda.synchronize()
                scale = x.abs().max().item() * np.abs(h).sum()
                d1 = (yc - y).abs().max().item() / scale
                d2 = (yt - y).abs().max().item() / scale
                gs = a.rows * a.len / 1e9
                rec = {"dtype": str(dtype).split(".")[1], "N": n, "P": p, "hop": hop, "rows": a.rows, "len": a.len,
                       "fused_ms": t_fused * 1e3, "fused_gsps": gs / t_fused, "fused_alg_tbs": alg / t_fused / 1e12,
                       "composed_ms": t_comp * 1e3, "composed_gsps": gs / t_comp,
                       "torch_ms": t_torch * 1e3, "torch_gsps": gs / t_torch,
                       "speedup_vs_composed": t_comp / t_fused, "maxdiff_composed": d1, "maxdiff_torch": d2}
                print(f"{rec['dtype']} N={n:5d} P={p:5d} hop={hop:5d}: fused {rec['fused_gsps']:7.2f} GS/s "
                      f"{rec['fused_alg_tbs']:5.2f} TB/s | composed {rec['composed_gsps']:6.2f} GS/s "
                      f"(x{rec['speedup_vs_composed']:5.1f}) | torch {rec['torch_gsps']:6.2f} GS/s | "
                      f"diff {d1:.1e} {d2:.1e}", flush=True)
                if out:
                    out.write(json.dumps(rec) + "\n")
                    out.flush()
                del f, y, xp, idx
            plan.close()
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

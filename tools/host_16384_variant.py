"""Which kernel should the host boundary run for f64 real rows of N = 16384?  Times pdsp_fft_transform_host_f64
(real rows, f64 mode, PDSP_HOST_THREADS as the caller has it) at 1, 7, 8, 64 and 512 rows: f64 rows in host memory ->
f64 planes in host memory, staging and PCIe included (never bench.py's `value`).  One process times one variant; run
the variants alternately, and the same one repeatedly, to see the run-to-run spread (profiles/host_16384_variant.jsonl).

    python tools/host_16384_variant.py --label packed                     # the library's host rule
    python tools/host_16384_variant.py --label fourstep --real-packed 0    # pdsp_set_real_packed(0): the four-step path
    PDSP_LIB_PATH=other/libpdsp_hip.so python tools/host_16384_variant.py --label parent

Prints one JSON line per row count: the median and the minimum over --samples samples, each the mean of enough calls to
last --window seconds."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pragma_dsp_amd  # noqa: E402,F401
from pragma_dsp_amd._capi import check, dptr, lib  # noqa: E402

N = 16384


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", required=True)
    ap.add_argument("--real-packed", type=int, default=1)
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 7, 8, 64, 512])
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--window", type=float, default=0.05)
    a = ap.parse_args()
    lib.pdsp_set_host_precision(64)
    lib.pdsp_set_real_packed(a.real_packed)
    plan = C.c_void_p()
    check(lib.pdsp_plan_create(N, -1, C.byref(plan)))
    rng = np.random.default_rng(1337)
    for rows in a.rows:
        re = rng.standard_normal((rows, N))
        ore, oim = np.empty_like(re), np.empty_like(re)

        def call():
            check(lib.pdsp_fft_transform_host_f64(plan, rows, N, dptr(re), None, dptr(ore), dptr(oim), 0))

        for _ in range(5):  # plan tables, staging, streams, code objects
            call()
        t0 = time.perf_counter()
        call()
        k = max(1, int(a.window / max(time.perf_counter() - t0, 1e-6)))
        samples = []
        for _ in range(a.samples):
            t0 = time.perf_counter()
            for _ in range(k):
                call()  # synchronous: returns after the results are in host memory
            samples.append((time.perf_counter() - t0) / k)
        print(json.dumps({"op": "fft_transform_host_f64 real rows", "n": N, "precision": 64, "label": a.label, "rows": rows,
                          "real_packed": a.real_packed, "host_threads": os.environ.get("PDSP_HOST_THREADS", "default"),
                          "calls_per_sample": k, "us_median": float(np.median(samples)) * 1e6,
                          "us_min": min(samples) * 1e6, "us_max": max(samples) * 1e6,
                          "checksum": float(ore[0, :64].sum() + oim[-1, :64].sum())}), flush=True)
    lib.pdsp_plan_destroy(plan)


if __name__ == "__main__":
    main()

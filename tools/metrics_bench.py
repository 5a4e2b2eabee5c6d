"""Time of the validation metrics (K.hdr_metrics = shdr_pair_moments_f32 + shdr_hdr_metrics_f32) against the HBM floor of their
compulsory traffic: both images read once per launch, 24 B per pixel, at the measured 6.29 TB/s.

Per size: after --warmup calls, each launch is timed with device events around --iters back-to-back calls on one stream (one
synchronise at the end), repeated --repeats times; the median per-call time is reported with the spread.  One JSON line.

    python tools/metrics_bench.py [--sizes 16x512x512,4x1024x1024] [--iters 200] [--repeats 5] [--warmup 20]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pkg = importlib.import_module("singlehdr-tf2_amd")
K, L = pkg._ops, pkg._lib
HBM_BYTES_PER_S = 6.29e12


def timed(fn, iters, repeats, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        t1.synchronize()
        us.append(t0.elapsed_time(t1) * 1e3 / iters)
    return float(np.median(us)), [round(u, 2) for u in us]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16x512x512,4x1024x1024")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench.py needs a HIP device")
    lib = L.load()
    out = {"hbm_bytes_per_s": HBM_BYTES_PER_S, "tile": list(K.METRICS_TILE), "sizes": {}}
    for size in a.sizes.split(","):
        n, h, w = (int(v) for v in size.split("x"))
        g = torch.Generator(device="cuda").manual_seed(0)
        gt = torch.rand((n, h, w, 3), device="cuda", generator=g) * 4.0
        pred = gt * (1.0 + 0.05 * torch.randn((n, h, w, 3), device="cuda", generator=g))
        ws = torch.empty(lib.shdr_metrics_workspace_bytes(n, h, w) // 8, device="cuda", dtype=torch.float64)
        o = torch.empty((7, n), device="cuda", dtype=torch.float64)
        p = K._ptr

        def moments():
            L.check(lib.shdr_pair_moments_f32(p(pred), p(gt), n, h, w, 1, p(o[4]), p(o[5]), p(o[6]), p(ws), K._stream()), "moments")

        def fused():
            L.check(lib.shdr_hdr_metrics_f32(p(pred), p(gt), n, h, w, 5000.0, p(o[4]), p(o[5]), p(o[6]), p(o[0]), p(o[1]), p(o[2]),
                                             p(o[3]), p(ws), K._stream()), "metrics")

        floor_us = 24.0 * n * h * w / HBM_BYTES_PER_S * 1e6
        row = {"floor_us_per_launch": round(floor_us, 2)}
        for name, fn in (("pair_moments", moments), ("hdr_metrics", fused), ("both_via_K", lambda: K.hdr_metrics(pred, gt))):
            us, runs = timed(fn, a.iters, a.repeats, a.warmup)
            row[name] = {"us": round(us, 2), "runs_us": runs,
                         "fraction_of_floor": round(floor_us * (2 if name == "both_via_K" else 1) / us, 4)}
        out["sizes"][size] = row
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

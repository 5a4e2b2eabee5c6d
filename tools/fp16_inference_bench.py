#!/usr/bin/env python3
"""fp32 vs native-fp16 inference (`pipeline.Inference(..., precision=...)`) at BASELINE configs[2]: 16 x 512^2, deq + lin + hal,
weights as bench.py makes them (Keras initialisers, BatchNorm statistics randomised).  The two precisions alternate in ONE process:
per window, `--steps` forwards of one precision between two device events, ending in a synchronise; the images/s of each precision
is the median over `--windows` windows, after `--warmup` forwards each.  Also reported: max |fp16 - fp32| / max |fp32| of the outputs
(tensor scale).  --ref adds the Refinement-Net (its input packed as fp16 [A, B, C, 0...] under fp16).  One JSON line on stdout.

    python tools/fp16_inference_bench.py [--batch 16] [--size 512] [--steps 5] [--windows 5] [--ref] [--only fp16]

--only PREC runs that precision alone (for a kernel trace: rocprofv3 --kernel-trace --stats -- python tools/fp16_inference_bench.py
--only fp16 --windows 1)."""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def randomise_bn(model, gen):
    """the weights of bench.py: BN moving stats mu~N(0,0.1), var~U(0.5,1.5), gamma/beta non-trivial"""
    with torch.no_grad():
        for name, t, _ in model.named_weights():
            if name.endswith(".moving_mean") or name.endswith(".beta"):
                t.copy_(torch.randn(t.shape, generator=gen) * 0.1)
            elif name.endswith(".moving_variance") or name.endswith(".gamma"):
                t.copy_(torch.rand(t.shape, generator=gen) + 0.5)
            elif name.endswith(".bias"):
                t.copy_(torch.randn(t.shape, generator=gen) * 0.05)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5, help="forwards per timed window")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per precision (median)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--streams", type=int, default=2, help="batch slices on this many HIP streams (bench.py's default)")
    ap.add_argument("--ref", action="store_true", help="also run the Refinement-Net")
    ap.add_argument("--only", choices=("fp32", "fp16"), help="run one precision alone")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    pkg = importlib.import_module("singlehdr-tf2_amd")
    torch.manual_seed(1234)
    gen = torch.Generator().manual_seed(4321)
    nets = [pkg.dequantization_net.model(), pkg.linearization_net.model(), pkg.hallucination_net.model()]
    nets.append(pkg.refinement_net.model() if args.ref else None)
    for m in nets:
        if m is not None:
            randomise_bn(m, gen)
    precs = [args.only] if args.only else ["fp32", "fp16"]
    runs = {p: pkg.pipeline.Inference(*nets, streams=args.streams, precision=p) for p in precs}
    g = torch.Generator().manual_seed(3)
    ldr = (torch.round(torch.rand((args.batch, args.size, args.size, 3), generator=g) * 255.0) / 255.0).cuda()

    outs = {}
    for p in precs:
        for _ in range(args.warmup):
            outs[p] = runs[p](ldr)
    torch.cuda.synchronize()
    times = {p: [] for p in precs}
    for _ in range(args.windows):
        for p in precs:                                    # alternated: clocks and thermals drift over both alike
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(args.steps):
                outs[p] = runs[p](ldr)
            t1.record()
            torch.cuda.synchronize()
            times[p].append(t0.elapsed_time(t1) / 1e3)
    res = {"workload": "deq+lin+hal%s inference, batch %d x %dx%d, %d streams" % ("+ref" if args.ref else "", args.batch, args.size,
                                                                                  args.size, args.streams),
           "windows": args.windows, "steps_per_window": args.steps}
    for p in precs:
        med = statistics.median(times[p])
        res[p] = {"images_per_s": round(args.batch * args.steps / med, 2), "ms_per_step": round(med / args.steps * 1e3, 2),
                  "window_spread": round((max(times[p]) - min(times[p])) / med, 4), "finite": bool(torch.isfinite(outs[p]).all())}
    if len(precs) == 2:
        a, b = outs["fp16"].double(), outs["fp32"].double()
        res["fp16_max_rel_diff"] = float((a - b).abs().max() / b.abs().max())
        res["speedup"] = round(res["fp16"]["images_per_s"] / res["fp32"]["images_per_s"], 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The Hallucination-Net's u1 (256^2 -> 512^2, 128 -> 64, projected to 3 channels) in the one-launch low-res form (csrc/up2_fused.hip)
against today's form (SHDR_NO_UP2_FUSED=1: the bilinear prologue inside conv_x3_kernel with the projection in its epilogue), same process,
arms alternating, ROUNDS timings of REPS launches each per arm:
    python tools/up2_fused_ab.py [ROUNDS]
Prints per batch size (16 and 8) the fastest and slowest round of each arm, the ratio of the medians, whether the ranges are apart, and the
largest difference of the two results over the output maximum."""
import importlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
shdr = importlib.import_module("singlehdr-tf2_amd")
K = shdr._ops
LIB = shdr._lib.load()

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
REPS = 10
H, W, CIN, COUT = 256, 256, 128, 64


def arm(fused):
    if fused:
        os.environ.pop("SHDR_NO_UP2_FUSED", None)
    else:
        os.environ["SHDR_NO_UP2_FUSED"] = "1"
    LIB.shdr_config_reload()


def timeit(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


print("u1 %dx%d x2 %d->%d projected, %d rounds of %d launches per arm; ms per launch: fastest .. slowest round" % (H, W, CIN, COUT, ROUNDS, REPS))
with torch.no_grad(), K.range_scope():
    for n in (16, 8):
        x = torch.randn(n, H, W, CIN, device="cuda")
        K.absmax_slot(x)
        wt = (torch.randn(3, 3, CIN, COUT, device="cuda") / (3 * CIN ** 0.5)).requires_grad_(True)
        b, sc, sh = torch.randn(COUT, device="cuda"), torch.rand(COUT, device="cuda") + 0.5, torch.randn(COUT, device="cuda")
        proj = torch.randn(3, COUT, device="cuda")
        fn = lambda: K.conv2d_up2(x, wt, b, act1=K.ACT_RELU, scale=sc, shift=sh, act2=K.ACT_RELU, proj=proj, lowres=True)
        t = {True: [], False: []}
        out = {}
        for fused in (True, False):
            arm(fused)
            for _ in range(3):
                out[fused] = fn()
        for _ in range(ROUNDS):
            for fused in (True, False):
                arm(fused)
                t[fused].append(timeit(fn))
        arm(True)
        diff = ((out[True] - out[False]).abs().max() / out[False].abs().max()).item()
        mn, mo = statistics.median(t[True]), statistics.median(t[False])
        print("N %2d  fused %6.3f .. %6.3f  today %6.3f .. %6.3f  today/fused %5.3f  %s  max diff / max %.2g"
              % (n, min(t[True]), max(t[True]), min(t[False]), max(t[False]), mo / mn,
                 "separated" if max(t[True]) < min(t[False]) else ("SLOWER" if min(t[True]) > max(t[False]) else "overlap"), diff), flush=True)

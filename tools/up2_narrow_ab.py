#!/usr/bin/env python3
"""The four `up.conv1` layers of the Dequantization-Net (bias + leaky relu behind a 2x bilinear up-sampling) on the low-res forms --
K.conv2d_up2(lowres=True, one_launch=True): csrc/up2_fused.hip in one launch for u1, u2 and u3, csrc/up2_lowres.hip in two for u4 -- against today's
call (the bilinear prologue inside the direct kernels), same process, arms alternating, ROUNDS timings of REPS launches each per arm:
    python tools/up2_narrow_ab.py [ROUNDS]
Prints per layer and batch size (16 and 8, the two-stream slice) the fastest and slowest round of each arm, the ratio of the medians,
whether the ranges are apart, and the largest difference of the two results over the output maximum."""
import importlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
shdr = importlib.import_module("singlehdr-tf2_amd")
K = shdr._ops

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
REPS = 10
LAYERS = [("u1", 256, 32, 16), ("u2", 128, 64, 32), ("u3", 64, 128, 64), ("u4", 32, 256, 128)]      # name, low-res side, Cin, Cout


def timeit(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


print("Dequantization-Net up.conv1, %d rounds of %d launches per arm; ms per layer: fastest .. slowest round" % (ROUNDS, REPS))
with torch.no_grad(), K.range_scope():
    for name, side, cin, cout in LAYERS:
        for n in (16, 8):
            x = torch.randn(n, side, side, cin, device="cuda")
            K.absmax_slot(x)
            wt = (torch.randn(3, 3, cin, cout, device="cuda") / (3 * cin ** 0.5)).requires_grad_(True)
            b = torch.randn(cout, device="cuda")
            arms = {True: lambda: K.conv2d_up2(x, wt, b, act1=K.ACT_LRELU, lowres=True, one_launch=True), False: lambda: K.conv2d_up2(x, wt, b, act1=K.ACT_LRELU)}
            t = {True: [], False: []}
            out = {}
            for low in (True, False):
                for _ in range(3):
                    out[low] = arms[low]()
            for _ in range(ROUNDS):
                for low in (True, False):
                    t[low].append(timeit(arms[low]))
            diff = ((out[True] - out[False]).abs().max() / out[False].abs().max()).item()
            mn, mo = statistics.median(t[True]), statistics.median(t[False])
            print("%s %3d^2 %3d->%3d N %2d  lowres %6.3f .. %6.3f  today %6.3f .. %6.3f  today/lowres %5.3f  %s  max diff / max %.2g"
                  % (name, side, cin, cout, n, min(t[True]), max(t[True]), min(t[False]), max(t[False]), mo / mn,
                     "separated" if max(t[True]) < min(t[False]) else ("SLOWER" if min(t[True]) > max(t[False]) else "overlap"), diff), flush=True)
            del x, out

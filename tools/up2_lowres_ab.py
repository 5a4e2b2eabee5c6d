#!/usr/bin/env python3
"""The Hallucination-Net `up` layers with the channel mix at low resolution (csrc/up2_lowres.hip: conv_x3_1x1_kernel + the stencil pass)
against today's form (SHDR_NO_UP2_LOWRES=1: the bilinear prologue inside conv_x3_wide_kernel, resize2x + plain at 512 couts), same
process, arms alternating, ROUNDS timings of REPS launches each per arm:
    python tools/up2_lowres_ab.py [N [ROUNDS]]
Prints per layer the fastest and slowest round of each arm, the ratio of the medians, the largest difference of the two results over the
output maximum, and -- from the kernel durations torch.profiler reports -- the GEMM and the stencil pass on their own with the stencil
pass's achieved bytes per second (z read once, y written once).  Both arms run with SHDR_X3_MIN_BLOCKS=1 so that every layer is measured."""
import importlib
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
shdr = importlib.import_module("singlehdr-tf2_amd")
K = shdr._ops
LIB = shdr._lib.load()

N = int(sys.argv[1]) if len(sys.argv) > 1 else 16
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
REPS = 10
SHAPES = [("u5", 16, 16, 512, 512), ("u4", 32, 32, 512, 512), ("u3", 64, 64, 512, 256), ("u2", 128, 128, 256, 128)]   # low-res h, w, cin, cout


def arm(lowres):
    if lowres:
        os.environ.pop("SHDR_NO_UP2_LOWRES", None)
    else:
        os.environ["SHDR_NO_UP2_LOWRES"] = "1"
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


def kernel_ms(fn):
    """mean device time per launch of every kernel of fn, by name"""
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        for _ in range(REPS):
            fn()
        torch.cuda.synchronize()
    out = {}
    for e in prof.key_averages():
        out[e.key] = e.device_time_total / 1e3 / REPS
    return out


os.environ["SHDR_X3_MIN_BLOCKS"] = "1"
print("N = %d, %d rounds of %d launches per arm; ms per launch: fastest .. slowest round" % (N, ROUNDS, REPS))
with torch.no_grad(), K.range_scope():
    for name, h, w, c, cout in SHAPES:
        x = torch.randn(N, h, w, c, device="cuda")
        K.absmax_slot(x)
        wt = (torch.randn(3, 3, c, cout, device="cuda") / (3 * c ** 0.5)).requires_grad_(True)
        b, sc, sh = torch.randn(cout, device="cuda"), torch.rand(cout, device="cuda") + 0.5, torch.randn(cout, device="cuda")
        fn = lambda: K.conv2d_up2(x, wt, b, act1=K.ACT_RELU, scale=sc, shift=sh, act2=K.ACT_RELU, lowres=True)
        t = {True: [], False: []}
        out = {}
        for lowres in (True, False):
            arm(lowres)
            for _ in range(3):
                out[lowres] = fn()
        for _ in range(ROUNDS):
            for lowres in (True, False):
                arm(lowres)
                t[lowres].append(timeit(fn))
        diff = ((out[True] - out[False]).abs().max() / out[False].abs().max()).item()
        arm(True)
        km = kernel_ms(fn)
        gemm = sum(v for k, v in km.items() if "conv_x3_1x1_kernel" in k)
        sten = sum(v for k, v in km.items() if "up2_lowres_stencil_kernel" in k)
        nbytes = 4.0 * N * h * w * cout * (9 + 4)
        mn, mo = statistics.median(t[True]), statistics.median(t[False])
        print("%s %3dx%-3d x2 %3d->%-3d  lowres %6.3f .. %6.3f  today %6.3f .. %6.3f  today/lowres %5.3f  %s  max diff / max %.2g  |  GEMM %6.3f ms %5.0f TF"
              "  stencil %6.3f ms %5.2f TB/s"
              % (name, h, w, c, cout, min(t[True]), max(t[True]), min(t[False]), max(t[False]), mo / mn,
                 "separated" if max(t[True]) < min(t[False]) else ("SLOWER" if min(t[True]) > max(t[False]) else "overlap"), diff,
                 gemm, 2.0 * N * h * w * c * 9 * cout / (gemm * 1e-3) / 1e12 if gemm else 0.0, sten, nbytes / (sten * 1e-3) / 1e12 if sten else 0.0),
              flush=True)

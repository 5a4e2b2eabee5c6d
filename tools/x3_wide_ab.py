#!/usr/bin/env python3
"""The plain 3x3 layers with a multiple of 128 couts on the 128-cout blocks (conv_x3_wide_kernel) against the 64-cout kernel
(SHDR_X3_SLICED=1), same process, arms alternating, ROUNDS timings of REPS launches each per arm:
    python tools/x3_wide_ab.py [N [ROUNDS]]
Prints per layer the fastest and slowest round of each arm (the spread of repeated launches of the same code) and the ratio of the
medians; the wide arm runs with SHDR_X3_WIDE_MIN_BLOCKS=1 and SHDR_X3_WIDE_MIN_COUT=128 so that every layer is measured, whatever the default thresholds."""
import contextlib
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
SHAPES = [  # h, w, c1, c2, cout: the hal encoder from d2.conv2 down, conv1, the decoder's 512-cout plain layers, a two-source layer
    (256, 256, 64, 0, 128), (256, 256, 128, 0, 128), (128, 128, 128, 0, 256), (128, 128, 256, 0, 256), (64, 64, 256, 0, 512),
    (64, 64, 512, 0, 512), (32, 32, 512, 0, 512), (16, 16, 512, 0, 512), (64, 64, 128, 128, 128), (128, 128, 512, 0, 256), (256, 256, 256, 0, 128),
]


def arm(sliced):
    if sliced:
        os.environ["SHDR_X3_SLICED"] = "1"
    else:
        os.environ.pop("SHDR_X3_SLICED", None)
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


os.environ["SHDR_X3_WIDE_MIN_BLOCKS"] = "1"
os.environ["SHDR_X3_WIDE_MIN_COUT"] = "128"
os.environ["SHDR_X3_MIN_BLOCKS"] = "1"
print("N = %d, %d rounds of %d launches per arm; ms per launch: fastest .. slowest round" % (N, ROUNDS, REPS))
with torch.no_grad(), (K.range_scope() if hasattr(K, "range_scope") else contextlib.nullcontext()):
    for h, w, c1, c2, cout in SHAPES:
        x = torch.randn(N, h, w, c1, device="cuda")
        x2 = torch.randn(N, h, w, c2, device="cuda") if c2 else None
        K.absmax_slot(x)
        if x2 is not None:
            K.absmax_slot(x2)
        wt = (torch.randn(3, 3, c1 + c2, cout, device="cuda") / (3 * (c1 + c2) ** 0.5)).requires_grad_(True)
        b = torch.randn(cout, device="cuda")
        fn = lambda: K.conv2d(x, wt, b, x2=x2, act1=K.ACT_RELU)
        t = {False: [], True: []}
        out = {}
        for sliced in (False, True):
            arm(sliced)
            assert K.conv2d_plan((N, h, w, c1), tuple(wt.shape), c2=c2) == "x3"
            for _ in range(3):
                out[sliced] = fn()
        for _ in range(ROUNDS):
            for sliced in (False, True):
                arm(sliced)
                t[sliced].append(timeit(fn))
        same = torch.equal(out[False].view(torch.int32), out[True].view(torch.int32))
        blocks = N * ((h + 15) // 16) * ((w + 15) // 16) * (cout // 128)
        mw, ms = statistics.median(t[False]), statistics.median(t[True])
        print("%3dx%-3d %3d+%-3d->%-3d %5d wide blocks  wide %6.3f .. %6.3f  sliced %6.3f .. %6.3f  sliced/wide %5.3f  %s  bits %s"
              % (h, w, c1, c2, cout, blocks, min(t[False]), max(t[False]), min(t[True]), max(t[True]), ms / mw,
                 "separated" if max(t[False]) < min(t[True]) else ("SLOWER" if min(t[False]) > max(t[True]) else "overlap"),
                 "equal" if same else "DIFFER"), flush=True)

# ---- the up-sampling layers: fused wide (conv_x3_wide_kernel<true>) / fused sliced / resize2x + plain (default dispatch of the plain layer)
UP_SHAPES = [(16, 16, 512, 512), (32, 32, 512, 512), (64, 64, 512, 256), (128, 128, 256, 128), (32, 32, 256, 128)]   # low-res h, w, cin, cout
os.environ["SHDR_X3_UP_ALWAYS"] = "1"        # the fused arms also at 512 couts
print("up-sampling layers, N = %d: fused wide / fused sliced / resize2x + plain conv (plain: default dispatch)" % N)
with torch.no_grad():
    for h, w, c, cout in UP_SHAPES:
        x = torch.randn(N, h, w, c, device="cuda")
        K.absmax_slot(x)
        wt = (torch.randn(3, 3, c, cout, device="cuda") / (3 * c ** 0.5)).requires_grad_(True)
        b = torch.randn(cout, device="cuda")
        fused = lambda: K.conv2d_up2(x, wt, b, act1=K.ACT_RELU)
        two = lambda: K.conv2d(K.resize2x(x), wt, b, act1=K.ACT_RELU)
        t = {"wide": [], "sliced": [], "two": []}
        out = {}
        for name, sliced, fn in (("wide", False, fused), ("sliced", True, fused)):
            arm(sliced)
            for _ in range(3):
                out[name] = fn()
        os.environ.pop("SHDR_X3_WIDE_MIN_BLOCKS"); os.environ.pop("SHDR_X3_WIDE_MIN_COUT"); arm(False)
        for _ in range(3):
            two()
        for _ in range(ROUNDS):
            os.environ["SHDR_X3_WIDE_MIN_BLOCKS"] = "1"; os.environ["SHDR_X3_WIDE_MIN_COUT"] = "128"
            arm(False); t["wide"].append(timeit(fused))
            arm(True); t["sliced"].append(timeit(fused))
            os.environ.pop("SHDR_X3_WIDE_MIN_BLOCKS"); os.environ.pop("SHDR_X3_WIDE_MIN_COUT")
            arm(False); t["two"].append(timeit(two))
        os.environ["SHDR_X3_WIDE_MIN_BLOCKS"] = "1"; os.environ["SHDR_X3_WIDE_MIN_COUT"] = "128"
        same = torch.equal(out["wide"].view(torch.int32), out["sliced"].view(torch.int32))
        blocks = N * ((2 * h + 15) // 16) * ((2 * w + 15) // 16) * (cout // 128)
        md = {k: statistics.median(v) for k, v in t.items()}
        print("%3dx%-3d x2 %3d->%-3d %5d wide blocks  wide %6.3f .. %6.3f  sliced %6.3f .. %6.3f  resize+plain %6.3f .. %6.3f  sliced/wide %5.3f  two/wide %5.3f  %s  bits %s"
              % (h, w, c, cout, blocks, min(t["wide"]), max(t["wide"]), min(t["sliced"]), max(t["sliced"]), min(t["two"]), max(t["two"]),
                 md["sliced"] / md["wide"], md["two"] / md["wide"],
                 "separated" if max(t["wide"]) < min(min(t["sliced"]), min(t["two"])) else "overlap or slower", "equal" if same else "DIFFER"), flush=True)

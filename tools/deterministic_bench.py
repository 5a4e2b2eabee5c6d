#!/usr/bin/env python3
"""Default against deterministic mode (`deterministic=True`, DESIGN.md section 4 "Deterministic mode") of the joint training step at
32 x 256^2 and of the fp32 fine-tuning step at 4 x 1024^2.  The two modes alternate in ONE process: per window `--steps` steps of one mode
between two device events, ending in a synchronise; the ms/step of a mode is the median over `--windows` windows, after `--warmup` steps
each.  The default mode IS the behaviour without this feature.  Also, per launch site at the shapes of the two workloads (`sites_ms`):
device-event times of the default call against the deterministic one (first launch + fold), `lin_frontend_bwd` scatter against gather
among them; and the workspace bytes a deterministic step allocates (sum and largest single call).  One JSON line on stdout.

    python tools/deterministic_bench.py [--steps 5] [--windows 5] [--warmup 2] [--only joint|finetune|sites] [--mode default|deterministic]

--mode runs one mode alone, for a kernel trace that shows the fold launches by name (col_fold_det_kernel, bn_fold_kernel,
lin_frontend_bwd_gather_kernel):  rocprofv3 --kernel-trace --stats -- python tools/deterministic_bench.py --only joint --mode deterministic
--windows 1"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def alternate(fns, args):
    """{name: median ms/step}: the modes alternate window by window"""
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.windows):
        for k, fn in fns.items():
            ms[k].append(timed(fn, args.steps))
    return {k: round(statistics.median(v), 3) for k, v in ms.items()}


def in_mode(step, deterministic, call):
    """ONE step object (one flat parameter buffer); the mode is its `deterministic` attribute, read at every call"""
    def fn():
        step.deterministic = deterministic
        call(step)
    return fn


def vgg_weights():
    """the VGG weights of bench.py"""
    vg = torch.Generator().manual_seed(99)
    dd = {}
    for name, cin, cout in (("conv1_1", 3, 64), ("conv1_2", 64, 64), ("conv2_1", 64, 128), ("conv2_2", 128, 128), ("conv3_1", 128, 256),
                            ("conv3_2", 256, 256), ("conv3_3", 256, 256)):
        lim = (6.0 / (9 * cin + 9 * cout)) ** 0.5
        dd[name] = [((torch.rand((3, 3, cin, cout), generator=vg) * 2 - 1) * lim).numpy(), torch.zeros(cout).numpy()]
    return dd


def site_times(K, args, g):
    """{site: {"default": ms, "deterministic": ms}} of single calls at the shapes of the two workloads"""
    def rnd(*shape):
        return torch.randn(shape, generator=g).cuda()
    sites = {}

    def wgrad(name, n, h, c1, cout, k, stride=1, c2=0):
        x, dz = rnd(n, h, h, c1), rnd(n, h // stride, h // stride, cout)
        x2 = rnd(n, h, h, c2) if c2 else None
        sites["wgrad " + name] = lambda: K.conv2d_wgrad(x, x2, dz, (k, k, c1 + c2, cout), stride, 1.0 / 255)
    wgrad("all-taps 7x7 16->16, 32x256^2", 32, 256, 16, 16, 7)
    wgrad("all-taps 3x3 32+32->32, 32x256^2", 32, 256, 32, 32, 3, c2=32)
    wgrad("MFMA 1x1 256+256->256, 32x64^2", 32, 64, 256, 256, 1, c2=256)
    wgrad("Winograd-domain 3x3 64->64, 32x256^2", 32, 256, 64, 64, 3)
    wgrad("split-operand 3x3 256->256, 32x64^2", 32, 64, 256, 256, 3)
    wgrad("split-operand 3x3 512->512, 32x32^2", 32, 32, 512, 512, 3)
    wgrad("split-operand 7x7/2 stem 96->64, 32x256^2", 32, 256, 96, 64, 7, stride=2)
    dy, y = rnd(32, 256, 256, 64), rnd(32, 256, 256, 64)
    sites["act_bwd_bias relu 32x256^2x64"] = lambda: K.act_bwd_bias(dy, y, K.ACT_RELU)
    d3 = rnd(32, 256, 256, 3)
    sites["bias_grad 32x256^2x3"] = lambda: K.bias_grad(d3)
    a3, b3 = torch.rand((32, 256, 256, 3), generator=g).cuda(), torch.rand((32, 256, 256, 3), generator=g).cuda()
    sites["diff_loss 32x256^2x3"] = lambda: K.diff_loss(a3, b3, 0)
    sites["tv_loss 32x256^2x3"] = lambda: K.tv_loss(a3)
    rf = torch.sort(torch.rand((32, 1024), generator=g), dim=1).values.cuda()
    sites["apply_rf_bwd 32x256^2x3, K 1024"] = lambda: K.apply_rf_bwd(a3, rf, d3, True)
    dinv, feat, wfc, table = rnd(32, 1024), rnd(32, 2048), rnd(2048, 11), rnd(1024, 12)
    sites["invcrf_decode_bwd B 32, F 2048"] = lambda: K.invcrf_decode_bwd(dinv, feat, wfc, table)
    img, dF = torch.rand((4, 1024, 1024, 3), generator=g).cuda(), rnd(4, 1024, 1024, 96)
    sites["lin_frontend_bwd 4x1024^2 (scatter / gather)"] = lambda: K.lin_frontend_bwd(img, dF)
    r4 = rnd(4, 1024, 1024, 3)
    sites["sample_dot 4x1024^2x3"] = lambda: K.sample_dot(r4, r4)

    def mode(fn, det):
        def run():
            with K.deterministic(det):
                fn()
        return run
    return {name: alternate({"default": mode(fn, False), "deterministic": mode(fn, True)}, args) for name, fn in sites.items()}


def workspace_bytes(K, fn):
    """(sum, largest) of the workspaces one deterministic step asks for"""
    sizes, orig = [], K._det_ws

    def spy(*a, **kw):
        t, n = orig(*a, **kw)
        sizes.append(n)
        return t, n
    K._det_ws = spy
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        K._det_ws = orig
    return {"calls": len(sizes), "sum_bytes": int(sum(sizes)), "largest_bytes": int(max(sizes))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("joint", "finetune", "sites"))
    ap.add_argument("--mode", choices=("default", "deterministic"), help="run one mode alone (kernel traces)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    pkg = importlib.import_module("singlehdr-tf2_amd")
    K, P = pkg._ops, pkg.pipeline
    torch.manual_seed(1234)
    g = torch.Generator().manual_seed(3)
    out = {}

    def img(b, s, c=3):
        return (torch.round(torch.rand((b, s, s, c), generator=g) * 255.0) / 255.0).cuda()
    def pick(modes):
        return {k: v for k, v in modes.items() if args.mode in (None, k)}
    if args.only in (None, "sites") and args.mode is None:
        out["sites_ms"] = site_times(K, args, g)
        torch.cuda.empty_cache()
    if args.only in (None, "joint"):
        b, s = 32, 256
        nets = [pkg.dequantization_net.model(), pkg.linearization_net.model(), pkg.hallucination_net.model()]
        vgg = pkg.vgg16.Vgg16(data_dict=vgg_weights())
        clipped = img(b, s)
        ds = (img(b, s), img(b, s), clipped, clipped * 1.5, torch.ones((b, 1, 1, 1)).cuda())
        inv = torch.cumsum(torch.rand((b, 1024), generator=g), 1)
        inv = (inv / inv[:, -1:]).cuda()
        step = P.JointTrainStep(*nets, vgg)
        modes = {"default": in_mode(step, False, lambda st: st(ds, inv, apply=False)),
                 "deterministic": in_mode(step, True, lambda st: st(ds, inv, apply=False))}
        out["joint_32x256_ms"] = alternate(pick(modes), args)
        if args.mode is None:
            before = K.order_dependent_launches()
            modes["default"]()
            out["joint_order_dependent_launches"] = K.order_dependent_launches() - before
            out["joint_workspace"] = workspace_bytes(K, modes["deterministic"])
        del step, modes, nets, vgg, ds
        torch.cuda.empty_cache()
    if args.only in (None, "finetune"):
        b, s = 4, 1024
        nets = [pkg.dequantization_net.model(), pkg.linearization_net.model(), pkg.hallucination_net.model(), pkg.refinement_net.model()]
        ldr, hdr = img(b, s), img(b, s) * 0.9 + 0.05
        step = P.FinetuneStep(*nets)
        modes = {"default": in_mode(step, False, lambda st: st(ldr, hdr, apply=False)),
                 "deterministic": in_mode(step, True, lambda st: st(ldr, hdr, apply=False))}
        out["finetune_4x1024_ms"] = alternate(pick(modes), args)
        if args.mode is None:
            out["finetune_workspace"] = workspace_bytes(K, modes["deterministic"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""Radiance .hdr output: float HDR image on the device -> scanline-RLE bytes on the host, by the host encoder and by the device
encoder, measured, not gated.

    python tools/hdr_write_bench.py [--out result.json]

Inputs, made on the device: 16 x 512 x 512, 1 x 512 x 512 and 1 x 4096 x 3072 float images, smooth content plus noise, and an
all-smooth variant of each (which compresses well).  One process, alternating windows (host route, device route, host, ...), the
median of 5 windows each, wall time from a synchronised start to the coded bytes on the host:
  host route    K.rgbe_encode -> copy of the RGBE pixels (4 B each) -> shdr_rgbe_rle_encode per image (hdr_io.rle_encode)
  device route  K.rgbe_encode -> K.rgbe_rle_encode (four launches) -> copy of the offsets and of the coded bytes
                (hdr_io.rle_encode_device)
and, from device events inside the library call, the time of each of the four launches of the device encoder.  The two routes'
bytes are compared before anything is timed."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
shdr = importlib.import_module("singlehdr-tf2_amd")
K, hdr_io = shdr._ops, shdr.hdr_io

WINDOWS = 5
STAGES = ("setup", "sizes", "scan", "write")


def content(n, h, w, noise, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32),
                            indexing="ij")
    imgs = []
    k = 1.0 if noise else 16.0                                          # the smooth variant varies slowly: mantissa bytes repeat
    for i in range(n):
        base = torch.stack((2.0 + 1.9 * torch.sin(xx / (37.0 * k) + i), 0.6 + 0.5 * torch.cos(yy / 23.0), (xx + yy) * (8.0 / (h + w))), dim=-1)
        if noise:
            base = base * (1.0 + noise * torch.randn(base.shape, device="cuda", generator=g))
        imgs.append(base.clamp_(min=0))
    return torch.stack(imgs).contiguous()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def host_route(x):
    rgbe = K.rgbe_encode(x).cpu().numpy()
    return [hdr_io.rle_encode(rgbe[i]) for i in range(rgbe.shape[0])]


def device_route(x):
    return hdr_io.rle_encode_device(K.rgbe_encode(x))


def measure(x):
    n, h, w, _ = x.shape
    a, b = host_route(x), device_route(x)                               # warm-up, and the bench measures an encoder that is right
    assert a == b, "device bytes differ from the host routine's"
    coded = sum(len(d) for d in a)
    host, dev, parts = [], [], {k: [] for k in ("rgbe_encode", "pixel_copy", "host_rle", "device_rle", "coded_copy")}
    stages = {k: [] for k in STAGES}
    for _ in range(WINDOWS):
        host.append(wall(lambda: host_route(x)))
        dev.append(wall(lambda: device_route(x)))
        # the parts of both routes, each from a synchronised start
        box = {}
        parts["rgbe_encode"].append(wall(lambda: box.__setitem__("rgbe", K.rgbe_encode(x))))
        parts["pixel_copy"].append(wall(lambda: box.__setitem__("host", box["rgbe"].cpu().numpy())))
        t0 = time.perf_counter()
        for i in range(n):
            hdr_io.rle_encode(box["host"][i])
        parts["host_rle"].append((time.perf_counter() - t0) * 1e3)
        parts["device_rle"].append(wall(lambda: box.__setitem__("coded", K.rgbe_rle_encode(box["rgbe"]))))
        data, off = box["coded"]
        parts["coded_copy"].append(wall(lambda: data[:int(off.cpu()[-1])].cpu()))
        ms = []
        K.rgbe_rle_encode(box["rgbe"], stage_ms=ms)
        for k, v in zip(STAGES, ms):
            stages[k].append(v)
    med = lambda v: statistics.median(v)
    return {"images": n, "height": h, "width": w, "raw_bytes": 4 * n * h * w, "coded_bytes": coded, "coded_over_raw": coded / (4.0 * n * h * w),
            "host_route_ms": med(host), "device_route_ms": med(dev), "parts_ms": {k: med(v) for k, v in parts.items()},
            "stage_event_ms": {k: med(v) for k, v in stages.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    result = {}
    for name, (n, h, w) in (("batch16_512", (16, 512, 512)), ("single_512", (1, 512, 512)), ("single_4096x3072", (1, 3072, 4096))):
        for kind, noise in (("noisy", 0.02), ("smooth", 0.0)):
            result["%s_%s" % (name, kind)] = measure(content(n, h, w, noise, seed=n + h))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

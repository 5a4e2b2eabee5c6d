"""Gain-map JPEG output: float HDR image and uint8 SDR image on the device -> finished files on the host, by the device route and by
the host-twin route, measured, not gated.

    python tools/ultrahdr_bench.py [--out result.json] [--factor 4]

Inputs, made on the device: 16 x 512 x 512, 1 x 512 x 512 and 1 x 4096 x 3072 pairs (a smooth SDR picture with noise, the HDR image
its linear values times a smooth gain).  One process, alternating windows (device, host twin, device, ...), the median of 5 windows
each, wall time from a synchronised start to the finished bytes on the host:
  device route     ultrahdr.encode(device tensors): K.gainmap_encode, jpeg.encode of the primaries and of the maps on the device
  host twin route  the same images brought to the host (.cpu(), inside the window), ultrahdr.encode(encoder="host")
and, from device events, the three launches of K.gainmap_encode (hdr_scale "auto") and the one of K.gainmap_apply beside their HBM
floors at 6.29 TB/s: encode reads 15 B / pixel once in the cell launch and 15 B / pixel in the statistics; apply reads 3 B / pixel and
writes 12 B / pixel.  Before anything is timed the device route's files are compared with the host twin route's (the small shapes)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
shdr = importlib.import_module("singlehdr-tf2_amd")
K, U = shdr._ops, shdr.ultrahdr

WINDOWS = 5
HBM_BYTES_PER_MS = 6.29e9                                               # 6.29 TB/s


def content(n, h, w, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32),
                            indexing="ij")
    table = torch.from_numpy(K.gainmap_math_host("srgb")).cuda()
    sdrs, hdrs = [], []
    for i in range(n):
        base = torch.stack((0.5 + 0.45 * torch.sin(xx / 37.0 + i), 0.5 + 0.4 * torch.cos(yy / 23.0), (xx + yy) / (h + w)), dim=-1)
        base = base + 0.02 * torch.randn(base.shape, device="cuda", generator=g)
        sdr = (base.clamp_(0, 1) * 255.0).round_().to(torch.uint8)
        gain = torch.exp2(2.0 + 2.0 * torch.sin(xx / 301.0) * torch.cos(yy / 211.0))[..., None]
        sdrs.append(sdr.contiguous())
        hdrs.append((table[sdr.long()] * gain).contiguous())
    return sdrs, hdrs


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events(fn, reps=5):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def measure(name, n, h, w, factor, check):
    sdrs, hdrs = content(n, h, w, 7)
    device = lambda: U.encode(hdrs, sdrs, factor=factor)
    host = lambda: U.encode([t.cpu().numpy() for t in hdrs], [t.cpu().numpy() for t in sdrs], factor=factor, encoder="host")
    files = device()                                                     # warm-up of every shape the windows use
    if check:
        assert files == host(), "the device route's files are not the host twin route's"
    t_dev, t_host = [], []
    for _ in range(WINDOWS):
        t_dev.append(wall(device))
        t_host.append(wall(host))
    pixels = n * h * w
    images, _, _ = K.gainmap_images([(h, w)] * n, factor)
    sdr_arena, hdr_arena = torch.cat([s.reshape(-1) for s in sdrs]), torch.cat([t.reshape(-1) for t in hdrs])
    stage = []
    for _ in range(WINDOWS):
        ms = []
        maps, meta = K.gainmap_encode(sdr_arena, hdr_arena, images, stage_ms=ms)
        stage.append(ms)
    stage = [statistics.median(col) for col in zip(*stage)]
    rec = meta.cpu().numpy().view(K.GAINMAP_META_DTYPE)
    mh, mw = -(-h // factor), -(-w // factor)
    items = [dict(height=h, width=w, factor=factor, map_channels=3, gain_min=r["gain_min"], gain_max=r["gain_max"]) for r in rec]
    ap, _ = K.gainmap_apply_images(items)
    K.gainmap_apply(sdr_arena, maps, ap)
    t_apply = events(lambda: K.gainmap_apply(sdr_arena, maps, ap))
    row = dict(shape=name, factor=factor, bytes=sum(len(f) for f in files), device_ms=statistics.median(t_dev), host_twin_ms=statistics.median(t_host),
               statistics_ms=stage[0], cells_ms=stage[1], quantise_ms=stage[2], encode_floor_ms=30.0 * pixels / HBM_BYTES_PER_MS,
               apply_ms=t_apply, apply_floor_ms=15.0 * pixels / HBM_BYTES_PER_MS, map=(mh, mw))
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--factor", type=int, default=4)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a HIP device"
    rows = [measure("16 x 512 x 512", 16, 512, 512, args.factor, True), measure("1 x 512 x 512", 1, 512, 512, args.factor, True),
            measure("1 x 4096 x 3072", 1, 3072, 4096, args.factor, False)]
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()

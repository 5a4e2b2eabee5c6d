"""Radiance .hdr input: files in the page cache -> RGBE pixels resident on the device, by the host decoder and by the device decoder,
measured, not gated.

    python tools/hdr_load_bench.py [--out result.json] [--dir scratch_dir]

Files are written once (hdr_io.write_hdr) and read back before anything is timed, so they come from the page cache.  Sets: 16 x 512 x 512,
1 x 512 x 512 and 1 x 4096 x 3072 (H = 3072), each noisy (long literals) and smooth (long runs).  One process, alternating windows
(host route, device route, host, ...), the median of 5 windows each, wall time from a synchronised start to the pixels on the device:
  host route    read + header walk + shdr_rgbe_rle_decode in a pool of 16 threads (dataset.py's), then one pageable upload of 4 B / pixel
                per file (what PatchHDRDataset._load does)
  device route  read + header walk (hdr_io.read_scanlines) in the same pool, ONE upload of the coded bytes, ONE K.rgbe_rle_decode, one
                read-back of the reports (hdr_io.rle_decode_device)
and the parts of both, each from a synchronised start; from device events inside the library call, the time of each of the four stages;
the HBM floor of the decode (coded bytes read once + 4 B / pixel written, at the 6.29 TB/s DESIGN.md section 10 uses).  Last, a
dataset.PatchHDRDataset load of the 16-file set with hdr_rle="host" and "device".  The two routes' pixels are compared first."""
import argparse
import concurrent.futures
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
shdr = importlib.import_module("singlehdr-tf2_amd")
K, hdr_io, dataset = shdr._ops, shdr.hdr_io, shdr.dataset

WINDOWS = 5
THREADS = 16
STAGES = ("mark", "parse", "rank", "expand")
HBM_BYTES_PER_MS = 6.29e9


def content(n, h, w, noise, seed):
    """RGBE images as the encoder's bench makes them: a smooth scene, with or without 2 % noise"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32),
                            indexing="ij")
    k = 1.0 if noise else 16.0
    out = []
    for i in range(n):
        base = torch.stack((2.0 + 1.9 * torch.sin(xx / (37.0 * k) + i), 0.6 + 0.5 * torch.cos(yy / 23.0), (xx + yy) * (8.0 / (h + w))), dim=-1)
        if noise:
            base = base * (1.0 + noise * torch.randn(base.shape, device="cuda", generator=g))
        out.append(K.rgbe_encode(base.clamp_(min=0).contiguous()))
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def pooled(fn, items):
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(THREADS, len(items))) as pool:
        return list(pool.map(fn, items))


def host_route(paths, device):
    return [torch.from_numpy(a).to(device) for a in pooled(hdr_io.read_rgbe, paths)]


def device_route(paths, device):
    return hdr_io.rle_decode_device(pooled(hdr_io.read_scanlines, paths), device)


def read_file(path):
    with open(path, "rb") as f:
        return f.read()


def measure(paths, device):
    a, b = host_route(paths, device), device_route(paths, device)          # warm-up, and the bench measures a decoder that is right
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "device pixels differ from the host routine's"
    lines = [hdr_io.read_scanlines(p) for p in paths]
    coded = sum(len(l.data) for l in lines)
    raw = sum(4 * l.height * l.width for l in lines)
    shapes = np.array([(l.height, l.width) for l in lines], dtype=np.int32)
    src_off = np.concatenate([[0], np.cumsum([len(l.data) for l in lines])]).astype(np.int64)
    blob = np.concatenate([np.frombuffer(l.data, dtype=np.uint8) for l in lines])
    host, dev = [], []
    parts = {k: [] for k in ("read", "header_walk", "host_decode_pool", "pixel_uploads", "coded_upload", "decode_call", "report_readback")}
    stages = {k: [] for k in STAGES}
    for _ in range(WINDOWS):
        host.append(wall(lambda: host_route(paths, device)))
        dev.append(wall(lambda: device_route(paths, device)))
        t0 = time.perf_counter()
        pooled(read_file, paths)
        t1 = time.perf_counter()
        pooled(hdr_io.read_scanlines, paths)
        t2 = time.perf_counter()
        pixels = pooled(lambda l: l.decode(), lines)
        t3 = time.perf_counter()
        parts["read"].append((t1 - t0) * 1e3)
        parts["header_walk"].append(max(0.0, (t2 - t1) - (t1 - t0)) * 1e3)         # read_scanlines reads as well
        parts["host_decode_pool"].append((t3 - t2) * 1e3)
        parts["pixel_uploads"].append(wall(lambda: [torch.from_numpy(p).to(device) for p in pixels]))
        box = {}
        parts["coded_upload"].append(wall(lambda: box.__setitem__("src", torch.from_numpy(blob).to(device))))
        parts["decode_call"].append(wall(lambda: box.__setitem__("out", K.rgbe_rle_decode(box["src"], src_off, shapes))))
        parts["report_readback"].append(wall(lambda: torch.stack([box["out"][2], box["out"][3]]).cpu()))
        ms = []
        K.rgbe_rle_decode(box["src"], src_off, shapes, stage_ms=ms)
        for k, v in zip(STAGES, ms):
            stages[k].append(v)
    med = statistics.median
    return {"files": len(paths), "height": int(shapes[0, 0]), "width": int(shapes[0, 1]), "raw_bytes": raw, "coded_bytes": coded,
            "coded_over_raw": coded / raw, "host_route_ms": med(host), "device_route_ms": med(dev),
            "parts_ms": {k: med(v) for k, v in parts.items()}, "stage_event_ms": {k: med(v) for k, v in stages.items()},
            "hbm_floor_ms": (coded + raw) / HBM_BYTES_PER_MS}


def dataset_load(d, names, device):
    out = {}
    for _ in range(WINDOWS):
        for opt in ("host", "device"):
            t0 = time.perf_counter()
            ds = dataset.PatchHDRDataset(d, names, True, device=device, hdr_rle=opt)
            out.setdefault(opt, []).append(dict(total=(time.perf_counter() - t0) * 1e3, **{k: v * 1e3 for k, v in ds.load_seconds.items()}))
            del ds
    return {opt: {k: statistics.median(r[k] for r in runs) for k in runs[0]} for opt, runs in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--dir")
    args = ap.parse_args()
    device = torch.device("cuda", torch.cuda.current_device())
    result = {}
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        for name, (n, h, w) in (("batch16_512", (16, 512, 512)), ("single_512", (1, 512, 512)), ("single_4096x3072", (1, 3072, 4096))):
            for kind, noise in (("noisy", 0.02), ("smooth", 0.0)):
                tag = "%s_%s" % (name, kind)
                paths = []
                for i, img in enumerate(content(n, h, w, noise, seed=n + h)):
                    paths.append(os.path.join(d, "%s_%02d.hdr" % (tag, i)))
                    hdr_io.write_hdr(paths[-1], img, encoder="device")
                result[tag] = measure(paths, device)
                if n > 1:
                    result["dataset_" + tag] = dataset_load(d, [os.path.basename(p) for p in paths], device)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""PNG output: uint8 RGB image on the device -> finished PNG files on the host, by PIL (libpng + zlib level 6, one thread) and by the
device encoder with both deflate choices, measured, not gated.

    python tools/png_write_bench.py [--out result.json]

Inputs, made on the device: 16 x 512 x 512, 1 x 512 x 512 and 1 x 4096 x 3072 images, noisy and smooth content.  One process,
alternating windows (PIL route, device lz, device huffman, PIL, ...), the median of 5 windows each, wall time from a synchronised
start to the finished bytes on the host:
  PIL route     copy of the pixels (3 B each) -> Image.save(buf, "PNG") per image, one thread
  device route  png.encode(encoder="device"): K.png_encode (csrc/png_enc.hip) -> copy of the offsets -> ONE copy of the finished files
and, from device events inside the library call, the time of each stage of the device encoder beside the HBM floor of the whole call:
the pixels read twice, the filtered stream written once and read once, the files written once, over 6.29 TB/s.  The device files are
read back by PIL and compared with the pixels before anything is timed; the sizes of the three routes' files are reported against
the raw pixels."""
import argparse
import importlib
import io
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
K, png = shdr._ops, shdr.png

WINDOWS = 5
HBM_BYTES_PER_MS = 6.29e9                                               # 6.29 TB/s


def content(n, h, w, noise, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32),
                            indexing="ij")
    imgs = []
    for i in range(n):
        base = torch.stack((0.5 + 0.45 * torch.sin(xx / 37.0 + i), 0.5 + 0.4 * torch.cos(yy / 23.0), (xx + yy) / (h + w)), dim=-1)
        if noise:
            base = base + noise * torch.randn(base.shape, device="cuda", generator=g)
        imgs.append((base.clamp_(0, 1) * 255.0).round_().to(torch.uint8))
    return torch.stack(imgs).contiguous()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def pil_route(x):
    from PIL import Image
    host = x.cpu().numpy()
    out = []
    for i in range(host.shape[0]):
        buf = io.BytesIO()
        Image.fromarray(host[i]).save(buf, "PNG")
        out.append(buf.getvalue())
    return out


def device_route(x, deflate):
    return png.encode(x, deflate=deflate)


def measure(x):
    from PIL import Image
    n, h, w, c = x.shape
    raw = n * h * w * c
    files = {"pil": pil_route(x), "lz": device_route(x, "lz"), "huffman": device_route(x, "huffman")}     # warm-up
    host = x.cpu().numpy()
    for d in ("lz", "huffman"):                                         # the bench measures an encoder that is right
        for i, data in enumerate(files[d]):
            assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), host[i]), "device file %d (%s) does not decode to its pixels" % (i, d)
    sizes = {k: sum(len(f) for f in v) for k, v in files.items()}
    walls = {k: [] for k in files}
    stages = {d: {k: [] for k in K.PNG_STAGE_NAMES} for d in ("lz", "huffman")}
    flat, shapes = x.reshape(-1), [(h, w, c)] * n
    for _ in range(WINDOWS):
        walls["pil"].append(wall(lambda: pil_route(x)))
        for d in ("lz", "huffman"):
            walls[d].append(wall(lambda: device_route(x, d)))
            ms = []
            K.png_encode(flat, shapes, "adaptive", d, stage_ms=ms)
            for k, v in zip(K.PNG_STAGE_NAMES, ms):
                stages[d][k].append(v)
    med = statistics.median
    stream = n * h * (w * c + 1)
    out = {"images": n, "height": h, "width": w, "raw_bytes": raw, "pil_route_ms": med(walls["pil"]),
           "file_over_raw": {k: v / raw for k, v in sizes.items()}}
    for d in ("lz", "huffman"):
        ev = {k: med(v) for k, v in stages[d].items()}
        out["device_%s" % d] = {"route_ms": med(walls[d]), "pil_over_device": med(walls["pil"]) / med(walls[d]), "stage_event_ms": ev,
                                "event_sum_ms": sum(ev.values()), "hbm_floor_ms": (2 * raw + 2 * stream + sizes[d]) / HBM_BYTES_PER_MS}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    torch.set_num_threads(1)
    result = {}
    for name, (n, h, w) in (("batch16_512", (16, 512, 512)), ("single_512", (1, 512, 512)), ("single_4096x3072", (1, 3072, 4096))):
        for kind, noise in (("noisy", 0.05), ("smooth", 0.0)):
            result["%s_%s" % (name, kind)] = measure(content(n, h, w, noise, seed=n + h))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Baseline-JPEG output: uint8 RGB image on the device -> finished JPEG files on the host, by PIL (libjpeg-turbo, one thread) and by
the device encoder, measured, not gated.

    python tools/jpeg_write_bench.py [--out result.json]

Inputs, made on the device: 16 x 512 x 512, 1 x 512 x 512 and 1 x 4096 x 3072 images, noisy and smooth content, 4:2:0, quality 90.
One process, alternating windows (PIL route, device route, PIL, ...), the median of 5 windows each, wall time from a synchronised
start to the finished bytes on the host:
  PIL route     copy of the pixels (3 B each) -> Image.save(buf, "JPEG", quality=90, subsampling=2) per image, one thread
  device route  jpeg.encode(encoder="device"): K.jpeg_encode (csrc/jpeg_enc.hip) into the buffers jpeg.encode keeps -> copy of the
                offsets and status words -> ONE copy of the finished files
and, from device events inside the library call, the time of each stage of the device encoder beside the stage's HBM floor: the bytes
the stage has to read and write (counted from the shapes and from the coded size, below) over 6.3 TB/s, the copy rate measured on
this chip.  The two routes' bytes are compared before anything is timed."""
import argparse
import importlib
import io
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
shdr = importlib.import_module("singlehdr-tf2_amd")
K, jpeg = shdr._ops, shdr.jpeg

WINDOWS = 5
QUALITY, SUBSAMPLING = 90, "420"
HBM_BYTES_PER_MS = 6.3e9                                                # 6.3 TB/s


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
        Image.fromarray(host[i]).save(buf, "JPEG", quality=QUALITY, subsampling=2)
        out.append(buf.getvalue())
    return out


def device_route(x):
    return jpeg.encode(x, quality=QUALITY, subsampling=SUBSAMPLING)


def floors(n, h, w, coded):
    """bytes each stage must move, from the shapes and the coded size (4:2:0: 6 blocks per 16 x 16 MCU)"""
    blocks = n * (-(-h // 16)) * (-(-w // 16)) * 6
    scan = coded - n * 625                                              # the unstuffed stream is about the coded scan
    moved = {"transform": 3 * n * h * w + 128 * blocks,                 # pixels in, int16 coefficients out
             "bits": 128 * blocks + 4 * blocks,                         # coefficients in, a count per block out
             "scan_segments": 4 * blocks + 8 * blocks,                  # counts in, int64 positions out
             "bit_stream": 128 * blocks + 8 * blocks + scan,            # coefficients and positions in, the stream out
             "ff_count_scan": scan,                                     # the stream in
             "sizes_scan": 0,                                           # per segment only
             "final": scan + coded}                                     # the stream in, the files out
    return {k: v / HBM_BYTES_PER_MS for k, v in moved.items()}


def measure(x):
    n, h, w, _ = x.shape
    a, b = pil_route(x), device_route(x)                                # warm-up, and the bench measures an encoder that is right
    assert a == b, "device bytes differ from PIL's"
    coded = sum(len(d) for d in a)
    desc = K.jpeg_enc_images([(h, w)] * n, QUALITY, SUBSAMPLING, 0)
    pil, dev = [], []
    parts = {k: [] for k in ("pixel_copy", "pil_encode", "device_encode", "coded_copy", "fresh_buffers")}
    sizes = {}
    K.jpeg_encode(x, desc, info=sizes)
    stages = {k: [] for k in K.JPEG_ENC_STAGE_NAMES}
    for _ in range(WINDOWS):
        pil.append(wall(lambda: pil_route(x)))
        dev.append(wall(lambda: device_route(x)))
        box = {}
        parts["pixel_copy"].append(wall(lambda: box.__setitem__("host", x.cpu().numpy())))
        t0 = time.perf_counter()
        from PIL import Image
        for i in range(n):
            Image.fromarray(box["host"][i]).save(io.BytesIO(), "JPEG", quality=QUALITY, subsampling=2)
        parts["pil_encode"].append((time.perf_counter() - t0) * 1e3)
        parts["device_encode"].append(wall(lambda: box.__setitem__("coded", K.jpeg_encode(x, desc))))
        data, off, _ = box["coded"]
        parts["coded_copy"].append(wall(lambda: data[:int(off.cpu()[-1])].cpu()))
        # what jpeg.encode saves by keeping its worst-case-sized output and workspace: allocating both anew
        parts["fresh_buffers"].append(wall(lambda: (torch.empty(sizes["out_bytes"], device="cuda", dtype=torch.uint8),
                                                    torch.empty(sizes["workspace_bytes"], device="cuda", dtype=torch.uint8))))
        ms = []
        K.jpeg_encode(x, desc, stage_ms=ms)
        for k, v in zip(K.JPEG_ENC_STAGE_NAMES, ms):
            stages[k].append(v)
    med = lambda v: statistics.median(v)
    return {"images": n, "height": h, "width": w, "raw_bytes": 3 * n * h * w, "coded_bytes": coded, "coded_over_raw": coded / (3.0 * n * h * w),
            "pil_route_ms": med(pil), "device_route_ms": med(dev), "pil_over_device": med(pil) / med(dev),
            "parts_ms": {k: med(v) for k, v in parts.items()}, "stage_event_ms": {k: med(v) for k, v in stages.items()},
            "stage_hbm_floor_ms": floors(n, h, w, coded)}


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

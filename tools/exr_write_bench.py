"""OpenEXR output: float HDR images on the device -> finished HALF / ZIP and HALF / PIZ files on the host, with the ZIP chunks deflated
by the host (zlib in a thread pool) and by the device (the Huffman-only encoder of csrc/deflate.hip and the LZ77 encoder of
csrc/deflate_lz.hip) and the PIZ chunks coded by the host (libshdr's encoder in the thread pool) and by the device (csrc/piz_enc.hip),
measured, not gated.

    python tools/exr_write_bench.py [--out result.json]

Inputs, made on the device: 16 x 512 x 512, 1 x 512 x 512 and 1 x 4096 x 3072 float images, a ramp with 2 % noise and a smooth variant
of each.  One process, alternating windows (host, device, device_lz, PIZ host, PIZ device, host, ...), the median of 5 windows each, wall
time from a synchronised start to the files' bytes on the host:
  host route       K.exr_pack -> copy of the predicted bytes -> zlib.compress per chunk (16 threads) -> assembly
  device route     K.exr_pack -> K.deflate_huffman (three launches) -> K.exr_finish_chunks -> copy of the offsets and of the finished bytes
  device_lz route  the same with K.deflate_lz (three launches: parse, scan, write)
  PIZ host route   K.exr_pack(lines=32) -> copy of the planar bytes -> K.piz_encode_host per chunk (16 threads) -> assembly
  PIZ device route K.exr_pack(lines=32) -> K.piz_encode (a memset and six launches) -> K.exr_finish_chunks -> the two copies
and the parts of all, each from a synchronised start, plus the device-event times of the encoders' launches.  All routes'
files are read back with exr.read_exr and compared with the HALF-rounded input before anything is timed."""
import argparse
import concurrent.futures
import importlib
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
shdr = importlib.import_module("singlehdr-tf2_amd")
K, exr = shdr._ops, shdr.exr

WINDOWS = 5
STAGES = ("stats", "scan", "write")
LZ_STAGES = ("parse", "scan", "write")


def content(n, h, w, noise, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(h, device="cuda", dtype=torch.float32), torch.arange(w, device="cuda", dtype=torch.float32),
                            indexing="ij")
    imgs = []
    for i in range(n):
        base = torch.stack((1.0 + xx / w + yy / h + 0.1 * i, 0.5 + 0.25 * xx / w + 0.1 * yy / h, 2.0 + 3.0 * (xx + yy) / (h + w)), dim=-1)
        if noise:
            base = base * (1.0 + noise * torch.randn(base.shape, device="cuda", generator=g))
        imgs.append(base)
    return torch.stack(imgs).contiguous()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def check(x, files, piz="refuse"):
    want = x[0].half().float()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "check.exr")
        with open(path, "wb") as f:
            f.write(files[0])
        assert torch.equal(exr.read_exr(path, piz=piz), want), "the file does not read back as the HALF-rounded input"


def measure(x):
    n, h, w, _ = x.shape
    host_files = exr.encode_exr(x, "half", "zip", "host")               # warm-up, and the bench measures encoders that are right
    dev_files = exr.encode_exr(x, "half", "zip", "device")
    lz_files = exr.encode_exr(x, "half", "zip", "device_lz")
    piz_host_files = exr.encode_exr(x, "half", "piz", piz="host")
    piz_files = exr.encode_exr(x, "half", "piz", piz="device")
    assert piz_files == piz_host_files, "the PIZ routes write different files"
    check(x, piz_files, piz="device")
    check(x, piz_files, piz="host")
    check(x, host_files)
    check(x, dev_files)
    check(x, lz_files)
    raw = 6 * n * h * w
    host, dev, lz, piz_host, piz_dev = [], [], [], [], []
    parts = {k: [] for k in ("pack", "predicted_copy", "host_deflate", "device_deflate", "device_lz_deflate", "finish", "finished_copy",
                             "lz_finished_copy", "piz_pack", "piz_encode", "piz_finished_copy")}
    piz_stages = {k: [] for k in K.PIZ_ENC_STAGE_NAMES}
    merge = []                                                          # per window: used symbols (max, mean) and merge ticks (max, mean) over the chunks
    stages = {k: [] for k in STAGES}
    lz_stages = {k: [] for k in LZ_STAGES}
    for _ in range(WINDOWS):
        host.append(wall(lambda: exr.encode_exr(x, "half", "zip", "host")))
        dev.append(wall(lambda: exr.encode_exr(x, "half", "zip", "device")))
        lz.append(wall(lambda: exr.encode_exr(x, "half", "zip", "device_lz")))
        piz_host.append(wall(lambda: exr.encode_exr(x, "half", "piz", piz="host")))
        piz_dev.append(wall(lambda: exr.encode_exr(x, "half", "piz", piz="device")))
        box = {}
        parts["pack"].append(wall(lambda: box.__setitem__("p", K.exr_pack(x, K.EXR_HALF, 16))))
        p = box["p"]
        n_chunks = p.chunk_off.size - 1
        parts["predicted_copy"].append(wall(lambda: box.__setitem__("host", p.predicted.cpu().numpy())))
        chunks = [box["host"][int(a):int(b)] for a, b in zip(p.chunk_off[:-1], p.chunk_off[1:])]
        t0 = time.perf_counter()
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(exr.MAX_DEFLATE_THREADS, n_chunks)) as pool:
            list(pool.map(zlib.compress, chunks))
        parts["host_deflate"].append((time.perf_counter() - t0) * 1e3)
        kw = dict(raw=p.planar, pad=8, front=8 * n_chunks, offsets_dev=p.chunk_off_dev)
        parts["device_deflate"].append(wall(lambda: box.__setitem__("z", K.deflate_huffman(p.predicted, p.chunk_off, **kw))))
        out, off, _ = box["z"]
        parts["finish"].append(wall(lambda: K.exr_finish_chunks(out, off, p, [300] * n)))
        parts["finished_copy"].append(wall(lambda: out[:8 * n_chunks + int(off.cpu()[-1])].cpu()))
        ms = []
        K.deflate_huffman(p.predicted, p.chunk_off, stage_ms=ms, **kw)
        for k, v in zip(STAGES, ms):
            stages[k].append(v)
        parts["device_lz_deflate"].append(wall(lambda: box.__setitem__("lz", K.deflate_lz(p.predicted, p.chunk_off, **kw))))
        lz_out, lz_off, _ = box["lz"]
        K.exr_finish_chunks(lz_out, lz_off, p, [300] * n)
        parts["lz_finished_copy"].append(wall(lambda: lz_out[:8 * n_chunks + int(lz_off.cpu()[-1])].cpu()))
        ms = []
        K.deflate_lz(p.predicted, p.chunk_off, stage_ms=ms, **kw)
        for k, v in zip(LZ_STAGES, ms):
            lz_stages[k].append(v)
        parts["piz_pack"].append(wall(lambda: box.__setitem__("q", K.exr_pack(x, K.EXR_HALF, 32, predict=False))))
        q = box["q"]
        q_chunks = q.chunk_off.size - 1
        geom, words = exr._piz_geometry(q, K.EXR_HALF)
        pkw = dict(pad=8, front=8 * q_chunks, chunk_off_dev=q.chunk_off_dev)
        parts["piz_encode"].append(wall(lambda: box.__setitem__("piz", K.piz_encode(q.planar, q.chunk_off, geom, words, **pkw))))
        p_out, p_off, _ = box["piz"]
        K.exr_finish_chunks(p_out, p_off, q, [300] * n)
        parts["piz_finished_copy"].append(wall(lambda: p_out[:8 * q_chunks + int(p_off.cpu()[-1])].cpu()))
        ms = []
        st = K.piz_encode(q.planar, q.chunk_off, geom, words, stage_ms=ms, stats=True, **pkw)[3].cpu().numpy()
        merge.append((int(st[:, 0].max()), float(st[:, 0].mean()), int(st[:, 1].max()), float(st[:, 1].mean())))
        for k, v in zip(K.PIZ_ENC_STAGE_NAMES, ms):
            piz_stages[k].append(v)
    med = statistics.median
    return {"images": n, "height": h, "width": w, "raw_bytes": raw, "chunks": n_chunks,
            "host_coded_over_raw": sum(len(f) for f in host_files) / raw, "device_coded_over_raw": sum(len(f) for f in dev_files) / raw,
            "device_lz_coded_over_raw": sum(len(f) for f in lz_files) / raw, "piz_coded_over_raw": sum(len(f) for f in piz_files) / raw,
            "piz_chunks": q_chunks, "host_route_ms": med(host), "device_route_ms": med(dev), "device_lz_route_ms": med(lz),
            "piz_host_route_ms": med(piz_host), "piz_device_route_ms": med(piz_dev),
            "piz_stage_event_ms": {k: med(v) for k, v in piz_stages.items()},
            "piz_merge": dict(zip(("symbols_max", "symbols_mean", "ticks_max", "ticks_mean"), (med(v) for v in zip(*merge)))),
            "parts_ms": {k: med(v) for k, v in parts.items()}, "stage_event_ms": {k: med(v) for k, v in stages.items()},
            "lz_stage_event_ms": {k: med(v) for k, v in lz_stages.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--only", help="one input by name, e.g. batch16_512_noisy")
    args = ap.parse_args()
    result = {}
    for name, (n, h, w) in (("batch16_512", (16, 512, 512)), ("single_512", (1, 512, 512)), ("single_4096x3072", (1, 3072, 4096))):
        for kind, noise in (("noisy", 0.02), ("smooth", 0.0)):
            if args.only and args.only != "%s_%s" % (name, kind):
                continue
            result["%s_%s" % (name, kind)] = measure(content(n, h, w, noise, seed=n + h))
            print(name, kind, json.dumps(result["%s_%s" % (name, kind)]), flush=True)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

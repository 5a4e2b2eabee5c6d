"""Time the training-set reader (dataset.py) on synthetic Radiance files (needs the GPU).

    python tools/synth_bench.py [--files 32] [--size 1024x1536] [--batch 32] [--iters 50] [--steps 6]

Prints one JSON line (and writes it to the file given by --out):
  load       files per second, split into host decode (file read + RLE decode, thread pool) and device time (upload,
             decode + resize kernel, crop means);
  assembly   the sampler launch for one batch of `--batch` 256^2 patches: median of event timings around the launch alone, and
             of read_batch_data() end to end (draws, pinned copy, launch, CRF / t gathers) up to a synchronise;
  joint      the joint step with reader + camera in the loop against the same step fed one fixed batch (bench.py --full's
             joint leg feeds fixed synthetic tensors), alternated in one process; medians of per-step wall times.
"""
import argparse
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

from oracle import imageio as O  # noqa: E402
from oracle import nets  # noqa: E402


def write_files(d, n, h, w, seed=0):
    pkg = importlib.import_module("singlehdr-tf2_amd")
    rng = np.random.default_rng(seed)
    for i in range(n):
        rgb = np.exp(rng.normal(0.0, 2.0, (h, w, 3))).astype(np.float32)
        rgb[: h // 4] = rgb[:1]                              # flat sky rows: real files have long runs
        pkg.hdr_io.write_hdr(os.path.join(d, "f%04d.hdr" % i), O.rgbe_encode(rgb))


def write_dorf(path, n=201, seed=0):
    rng = np.random.default_rng(seed)
    with open(path, "w") as f:
        for i in range(n):
            b = np.cumsum(rng.random(1024) + 0.01)
            b = (b - b[0]) / (b[-1] - b[0])
            f.write("curve-%d\ngraph\nI =\n%s\nB =\n%s\n" % (i, " ".join(["0"] * 1024), " ".join("%.9e" % v for v in b)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--size", default="1024x1536")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "synth_bench needs a HIP device"
    torch.cuda.set_device(0)
    pkg = importlib.import_module("singlehdr-tf2_amd")
    D = pkg.dataset
    h, w = (int(v) for v in args.size.split("x"))
    res = {"files": args.files, "file_size": [h, w], "batch": args.batch}
    with tempfile.TemporaryDirectory() as d:
        write_files(d, args.files, h, w)
        write_dorf(os.path.join(d, "dorfCurves.txt"))
        D.PatchHDRDataset(d, ["f0000.hdr"], True)            # warm-up: code objects, allocator
        ds = D.get_train_dataset(d, crf_path=os.path.join(d, "dorfCurves.txt"))
    patches = ds.dataset_list[0]
    ls = patches.load_seconds
    res["load"] = {"host_decode_s": round(ls["host_decode"], 4), "device_s": round(ls["device"], 4),
                   "files_per_s": round(args.files / (ls["host_decode"] + ls["device"]), 2),
                   "host_decode_files_per_s": round(args.files / ls["host_decode"], 2),
                   "device_files_per_s": round(args.files / ls["device"], 2),
                   "arena_mb": round(patches.arena.numel() * 4 / 2 ** 20, 1)}

    reader = D.RandDatasetReader(ds, args.batch, seed=1)
    params = torch.from_numpy(reader.draw()).cuda()
    K = pkg._ops
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
    for _ in range(3):
        K.hdr_patch_sample(patches.arena, patches.offsets, patches.dims, patches.means, params, 256)
    for a, b in ev:
        a.record()
        K.hdr_patch_sample(patches.arena, patches.offsets, patches.dims, patches.means, params, 256)
        b.record()
    torch.cuda.synchronize()
    kern = statistics.median(a.elapsed_time(b) for a, b in ev)
    wall = []
    for i in range(args.iters + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reader.read_batch_data()
        torch.cuda.synchronize()
        if i >= 3:
            wall.append((time.perf_counter() - t0) * 1e3)
    out_mb = args.batch * 256 * 256 * 12 / 1e6
    res["assembly"] = {"kernel_ms_median": round(kern, 4), "read_batch_data_ms_median": round(statistics.median(wall), 4),
                       "output_mb": round(out_mb, 2), "kernel_write_gb_per_s": round(out_mb / kern, 1)}

    P = {k: nets.init_params(getattr(nets, k + "_spec")(), 90 + i) for i, k in enumerate(("deq", "lin", "hal"))}
    V = nets.init_params(nets.vgg_spec(), 93)
    dd = {n: [V[n + ".kernel"], V[n + ".bias"]] for n in ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3")}
    step = pkg.pipeline.JointTrainStep(pkg.dequantization_net.model().load_numpy(P["deq"]),
                                       pkg.linearization_net.model().load_numpy(P["lin"]),
                                       pkg.hallucination_net.model().load_numpy(P["hal"]), pkg.vgg16.Vgg16(data_dict=dd))
    cam = pkg.camera.CameraPipeline(seed=2)
    hdr, crf, invcrf, t = reader.read_batch_data()
    fixed = (tuple(x.clone() for x in cam(hdr, crf, t)), invcrf.clone())

    def in_loop():
        hdr, crf, invcrf, t = reader.read_batch_data()
        return step(cam(hdr, crf, t), invcrf)

    def synthetic():
        return step(*fixed)

    for fn in (in_loop, synthetic):
        fn()
    times = {"in_loop": [], "synthetic": []}
    for _ in range(args.steps):
        for name, fn in (("in_loop", in_loop), ("synthetic", synthetic)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
            assert torch.isfinite(out["total"]).all(), name
    med = {k: statistics.median(v) for k, v in times.items()}
    res["joint"] = {"step_ms_reader_camera_in_loop": round(med["in_loop"], 2), "step_ms_fixed_batch": round(med["synthetic"], 2),
                    "overhead_ms": round(med["in_loop"] - med["synthetic"], 2), "steps": args.steps,
                    "samples_ms": {k: [round(x, 2) for x in v] for k, v in times.items()}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

"""Is the record route the bottleneck of fine-tuning on HDR-Real?  One process, one device:

  * a synthetic folder of --pairs pairs of --side x --side images is loaded once (HdrRealFolder.from_arrays: upload + the
    statistics launch, timed; device bytes per pair reported);
  * write_tfrecords makes the reference's GZIP records of it (timed, not part of either route);
  * batches per second of tfrecord.HdrRealDataset on those records and of HdrRealFolder on the folder, at every --batches size:
    after one warm-up window, the median of --windows windows of --window-batches (records) or --folder-window-batches
    (folder) batches, each ended by a stream synchronise (a window of the record route is cut short where its epoch ends);
  * beside them, the pipeline.FinetuneStep (fp32 and fp16) at 256 x 256, batch 4 that consumes the batches: the median step time.
One JSON line.

    python tools/hdr_real_bench.py [--pairs 16] [--side 512] [--batches 4,32] [--windows 5] [--window-batches 24]
                                   [--folder-window-batches 1000]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pkg = importlib.import_module("singlehdr-tf2_amd")


def synthetic_pair(rng, side):
    """a smooth scene with noise: mid-grey LDR (nothing for the filter to drop) and an HDR image of a few stops"""
    y, x = np.mgrid[0:side, 0:side].astype(np.float32) / side
    base = 0.5 + 0.3 * np.sin(6.0 * x + rng.random() * 6.0) * np.cos(5.0 * y + rng.random() * 6.0)
    ldr = np.clip(base[..., None] * 255.0 + rng.normal(0.0, 6.0, (side, side, 3)), 0, 255).astype(np.uint8)
    hdr = (np.exp2(4.0 * base[..., None]) * (1.0 + 0.05 * rng.standard_normal((side, side, 3)))).astype(np.float32)
    return ldr, hdr


def windows(next_batch, n_windows, window_batches):
    """median batches per second over n_windows windows after one warm-up window; next_batch() returns False at the end of the data"""
    rates = []
    for w in range(n_windows + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        done = 0
        while done < window_batches and next_batch():
            done += 1
        torch.cuda.synchronize()
        if w and done:
            rates.append(done / (time.perf_counter() - t0))
    return float(np.median(rates)), [round(r, 1) for r in rates]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--batches", default="4,32")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-batches", type=int, default=24, help="batches per window of the record route")
    ap.add_argument("--folder-window-batches", type=int, default=1000, help="batches per window of the folder route (a batch is one launch)")
    ap.add_argument("--step-precisions", default="fp32,fp16")
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    ldr, hdr = zip(*[synthetic_pair(rng, a.side) for _ in range(a.pairs)])
    H = pkg.hdr_real
    warm = H.HdrRealFolder.from_arrays(ldr[:1], hdr[:1])                   # first-launch costs are not the folder's
    del warm
    t0 = time.perf_counter()
    folder = H.HdrRealFolder.from_arrays(ldr, hdr)
    load_s = time.perf_counter() - t0
    out = {"pairs": a.pairs, "side": a.side, "kept_patches": len(folder.patches), "candidates": len(folder.candidates),
           "folder_load_and_stats_s": round(load_s, 4), "folder_device_s": round(folder.load_seconds["device"], 4),
           "device_bytes_per_pair": folder.device_bytes // a.pairs, "routes": {}, "finetune_step_256_b4_ms": {}}
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        paths = H.write_tfrecords(folder, d)
        out["write_tfrecords_s"] = round(time.perf_counter() - t0, 2)
        out["record_files"] = len(paths)
        out["record_mb_gzip"] = round(sum(os.path.getsize(p) for p in paths) / 1e6, 1)
        for b in [int(v) for v in a.batches.split(",") if v]:
            state = {"it": None}

            def next_record_batch():
                if state["it"] is None:
                    state["it"] = iter(pkg.tfrecord.HdrRealDataset(d, batch_size=b))
                try:
                    next(state["it"])
                    return True
                except StopIteration:
                    state["it"] = None                                     # the next window starts a new epoch
                    return False
            folder.batch_size = b

            def next_folder_batch():
                folder.render(folder.draw())
                return True
            rec, rec_all = windows(next_record_batch, a.windows, a.window_batches)
            fol, fol_all = windows(next_folder_batch, a.windows, a.folder_window_batches)
            out["routes"]["batch_%d" % b] = {"records_batches_per_s": round(rec, 1), "folder_batches_per_s": round(fol, 1),
                                             "records_ms_per_batch": round(1e3 / rec, 3), "folder_ms_per_batch": round(1e3 / fol, 3),
                                             "records_windows": rec_all, "folder_windows": fol_all}
    folder.batch_size = 4
    for prec in [p for p in a.step_precisions.split(",") if p]:
        torch.manual_seed(777)
        nets4 = [pkg.dequantization_net.model(), pkg.linearization_net.model(), pkg.hallucination_net.model(), pkg.refinement_net.model()]
        step = pkg.pipeline.FinetuneStep(*nets4, precision=prec, loss_scale=1.0 if prec == "fp32" else 0.25)
        ref_ldr, ref_hdr = folder.render(folder.draw())
        step(ref_ldr, ref_hdr)
        times = []
        for _ in range(a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(ref_ldr, ref_hdr)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        out["finetune_step_256_b4_ms"][prec] = round(float(np.median(times)) * 1e3, 2)
        del step, nets4
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

"""JPEG decode: PIL on one host thread (hdr_io.read_ldr) against the device decoder (jpeg.decode), measured, not gated.

    python tools/jpeg_bench.py [--out result.json]

Inputs, written with PIL into a temporary directory: 16 files of 512 x 512 at 4:2:0 quality 92 and one 4096 x 3072 file, smooth
content plus noise (not pure noise).  One process, alternating windows (PIL, device, PIL, ...), the median of 5 windows each.
jpeg.decode is timed end to end -- read, parse, unstuff, upload, kernels -- up to torch.cuda.synchronize.  Per candidate
subsequence length it also reports the wall time of the host half (plan: read + parse + unstuff + lay out; upload), the device
time of every stage of the library call from events recorded between the stages (shdr_jpeg_batch.stage_ms: clear, the
synchronisation passes with the host's waits between them, block scan + write pass, DC, IDCT, upsample + colour), the number
of synchronisation passes and the share of subsequences whose end state was final after the speculative decode (0 neighbours),
after one re-decode from the left neighbour (1), after two (2) and later.
The route with the scan prepared on the device (unstuff="device", csrc/jpeg_scan.hip) is measured in the same windows, right after
the host route of the same subsequence length: its end-to-end time, the wall time of the parts of its host half (read_parse, stage,
scan_launch, scan_wait, layout, compact_launch, upload), and the device-event times of the scan call and of the compaction call
beside their HBM floor: the raw bytes read twice and the arena written once at 6.29 TB/s."""
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
shdr = importlib.import_module("singlehdr-tf2_amd")
jpeg, hdr_io = shdr.jpeg, shdr.hdr_io

CANDIDATES = (256, 512, 1024, 2048)
WINDOWS = 5
HBM_BYTES_PER_MS = 6.29e9                                                  # the project's 6.29 TB/s figure


def content(seed, h, w):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([127 + 120 * np.sin(xx / 37.0 + seed), 127 + 120 * np.cos(yy / 23.0), (xx + yy) * 255.0 / (h + w)], axis=2)
    return np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def write(path, img):
    from PIL import Image
    Image.fromarray(img).save(path, "JPEG", quality=92, subsampling=2)
    return os.path.getsize(path)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def sync_shares(d):
    r = d.sync_rounds()
    r = r[r >= 0] % (jpeg.WG + 2) + (r[r >= 0] // (jpeg.WG + 2) > 0) * 1000       # later passes count as "more"
    n = float(r.size)
    return {"0": float((r == 0).sum() / n), "1": float((r == 1).sum() / n), "2": float((r == 2).sum() / n),
            "more": float((r > 2).sum() / n), "subsequences": int(n)}


def measure(paths):
    res = {"files": len(paths), "file_bytes": [os.path.getsize(p) for p in paths]}
    for bits in CANDIDATES:                                               # warm-up: code objects, allocator
        jpeg.decode(paths, subseq_bits=bits)
        jpeg.decode(paths, subseq_bits=bits, unstuff="device")
    pil, dev, scan = [], {b: [] for b in CANDIDATES}, {b: [] for b in CANDIDATES}
    for _ in range(WINDOWS):
        pil.append(wall(lambda: [hdr_io.read_ldr(p) for p in paths]))
        for bits in CANDIDATES:
            dev[bits].append(wall(lambda: jpeg.decode(paths, subseq_bits=bits)))
            scan[bits].append(wall(lambda: jpeg.decode(paths, subseq_bits=bits, unstuff="device")))
    res["pil_ms"] = statistics.median(pil)
    res["pil_upload_ms"] = statistics.median(
        wall(lambda: [torch.from_numpy(hdr_io.read_ldr(p)).cuda() for p in paths]) for _ in range(WINDOWS))
    res["device"] = {}
    for bits in CANDIDATES:
        runs = [jpeg.Decoded(paths, subseq_bits=bits, stages=True) for _ in range(WINDOWS)]
        d = runs[-1]
        med = lambda f: statistics.median(f(r) for r in runs)
        res["device"][str(bits)] = {
            "end_to_end_ms": statistics.median(dev[bits]),
            "host_ms": {k: med(lambda r: r.host_ms[k]) for k in ("plan", "upload")},            # wall: read + parse + unstuff; uploads
            "stage_event_ms": {k: med(lambda r: r.stage_ms[k]) for k in jpeg.STAGE_NAMES},       # device events inside the library call
            "passes": d.passes, "settled_after": sync_shares(d)}
    res["device_scan"] = {}
    for bits in CANDIDATES:
        plain = [jpeg.Decoded(paths, subseq_bits=bits, unstuff="device") for _ in range(WINDOWS)]      # host parts: no event waits inside
        timed = [jpeg.Decoded(paths, subseq_bits=bits, unstuff="device", stages=True) for _ in range(WINDOWS)]
        ev = timed[-1].scan_ms
        res["device_scan"][str(bits)] = {
            "end_to_end_ms": statistics.median(scan[bits]),
            "host_route_end_to_end_ms": statistics.median(dev[bits]),                            # the same windows
            "host_ms": {k: statistics.median(r.host_ms[k] for r in plain) for k in plain[0].host_ms},
            "scan_event_ms": statistics.median(r.scan_ms["scan"] for r in timed),
            "compact_event_ms": statistics.median(r.scan_ms["compact"] for r in timed),
            "stage_event_ms": {k: statistics.median(r.stage_ms[k] for r in timed) for k in jpeg.STAGE_NAMES},
            "raw_bytes": ev["raw_bytes"], "arena_bytes": ev["arena_bytes"],
            "hbm_floor_ms": (2 * ev["raw_bytes"] + ev["arena_bytes"]) / HBM_BYTES_PER_MS}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        small = [os.path.join(tmp, "s%02d.jpg" % i) for i in range(16)]
        for i, p in enumerate(small):
            write(p, content(i, 512, 512))
        large = os.path.join(tmp, "large.jpg")
        write(large, content(99, 3072, 4096))
        for p in small[:2] + [large]:                                    # the bench measures a decoder that is right
            assert np.array_equal(jpeg.decode([p])[0].cpu().numpy(), hdr_io.read_ldr(p)), p
            assert np.array_equal(jpeg.decode([p], unstuff="device")[0].cpu().numpy(), hdr_io.read_ldr(p)), p
        result = {"batch16_512": measure(small), "single_512": measure(small[:1]), "single_4096x3072": measure([large])}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

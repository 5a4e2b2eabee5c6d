"""Load time of the training-set reader on OpenEXR files: writes N synthetic ZIP (or ZIPS) files (HALF R, G, B, A; 3840 x 2160 by
default) to a temporary directory, builds PatchHDRDataset over them and prints its load_seconds (host decode: read + check, and
with the host route inflate, in the thread pool; device: upload, with the device route inflate, unpredict, load-resize, means), the
median of --repeat builds, as one JSON line.  The files are read from the page cache (they were just written).

    python tools/exr_load_bench.py [--files 8] [--width 3840] [--height 2160] [--repeat 3] [--compression zip|zips|piz]
                                   [--inflate host|device|both] [--piz host|device|both] [--out result.json]

--inflate both builds the dataset with exr_inflate="host" and "device" in alternating windows of one process, checks that the two
arenas are the same bits, and adds the parts of the device route, each from a synchronised start: read_stored in the thread pool,
the staging copy to the device, the K.inflate launch (device-event time), K.exr_unpredict; and the decode rate of ONE chunk alone
(one wave: the serial rate of the decoder) beside the rate of the whole launch.

--compression piz writes the files with the tests' PIZ writer (tests/piz_ref.py; one file is encoded, the others are copies of it:
the encoder is NumPy) and --piz chooses who decodes them: exr_piz="host" (libshdr's host decoder in the thread pool), "device"
(K.piz_decode) or both in alternating windows, with the arenas compared and the device route's parts: read_item in the pool for
both routes, upload_batch, the two launches' device-event times at several sub_bits, how many synchronisation rounds the
chunks took and the share of all subsequences that were final after round 0, 1, ... (those the next round did not decode again)."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import exr_ref as X  # noqa: E402
import piz_ref  # noqa: E402

pkg = importlib.import_module("singlehdr-tf2_amd")
K, exr, dataset = pkg._ops, pkg.exr, pkg.dataset


def _image(rng, h, w):
    """smooth gradients plus a little noise: compresses about as well as a rendered HDR frame"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.exp(2.0 * np.sin(x / 300.0) * np.cos(y / 200.0))
    return (base * (1.0 + 0.02 * rng.standard_normal((h, w)).astype(np.float32))).astype(np.float32)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def device_parts(paths, repeat):
    """the device route's parts in ms (medians), the chunk count and the decode rates"""
    dev = torch.device("cuda", torch.cuda.current_device())
    parts = {k: [] for k in ("read_stored_pool", "read_payload_pool", "upload_batch", "staging_copy", "inflate_event", "unpredict",
                             "one_chunk_event")}
    med = statistics.median
    for _ in range(repeat):
        box = {}
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(dataset.MAX_LOAD_THREADS, len(paths))) as pool:
            t0 = time.perf_counter()
            box["items"] = list(pool.map(exr.read_stored, paths))
            parts["read_stored_pool"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            list(pool.map(exr.read_payload, paths))
            parts["read_payload_pool"].append((time.perf_counter() - t0) * 1e3)
        items = box["items"]
        parts["upload_batch"].append(wall(lambda: exr.upload_batch(items, dev)))
        data = np.concatenate([it.data for it in items])
        src_off = np.concatenate([[0]] + [it.src_offsets[1:] + o for it, o in zip(items, np.cumsum([0] + [it.data.size for it in items]))])
        dst_off = np.concatenate([[0]] + [it.offsets[1:] + o for it, o in zip(items, np.cumsum([0] + [int(it.offsets[-1]) for it in items]))])
        mode = torch.from_numpy(np.concatenate([it.mode for it in items])).to(dev)
        pinned = torch.from_numpy(data).pin_memory()
        parts["staging_copy"].append(wall(lambda: box.__setitem__("src", pinned.to(dev, non_blocking=True))))
        ms = []
        out = K.inflate(box["src"], src_off, dst_off, mode=mode, stage_ms=ms)
        parts["inflate_event"].append(ms[0])
        off_dev = torch.from_numpy(dst_off).to(dev)
        parts["unpredict"].append(wall(lambda: K.exr_unpredict(out[0], off_dev, mode)))
        c = int(np.flatnonzero(np.concatenate([it.mode for it in items]))[0])                  # the first coded chunk, alone
        ms = []
        K.inflate(box["src"], src_off[c:c + 2], dst_off[c:c + 2] - dst_off[c], stage_ms=ms)
        parts["one_chunk_event"].append(ms[0])
    n_chunks, stored, decoded = src_off.size - 1, int(src_off[-1]), int(dst_off[-1])
    one_stored, one_decoded = int(src_off[c + 1] - src_off[c]), int(dst_off[c + 1] - dst_off[c])
    p = {k: round(med(v), 3) for k, v in parts.items()}
    return {"chunks": n_chunks, "stored_mb": round(stored / 1e6, 2), "decoded_mb": round(decoded / 1e6, 2), "parts_ms": p,
            "launch_decoded_mb_per_s": round(decoded / 1e6 / (p["inflate_event"] / 1e3), 1),
            "one_chunk": {"stored_bytes": one_stored, "decoded_bytes": one_decoded, "ms": p["one_chunk_event"],
                          "decoded_mb_per_s": round(one_decoded / 1e6 / (p["one_chunk_event"] / 1e3), 2)}}


def piz_device_parts(paths, repeat):
    """the PIZ device route's parts in ms (medians), the stage times per sub_bits and the rounds the chunks took"""
    dev = torch.device("cuda", torch.cuda.current_device())
    med = statistics.median
    parts = {k: [] for k in ("read_stored_pool", "read_host_pool", "upload_batch")}
    stages = {s: ([], []) for s in (128, 256, 1024, 4096, 16384)}
    rounds, final = {}, {}
    for _ in range(repeat):
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(dataset.MAX_LOAD_THREADS, len(paths))) as pool:
            t0 = time.perf_counter()
            items = list(pool.map(lambda p: exr.read_item(p, "host", "device"), paths))
            parts["read_stored_pool"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            list(pool.map(lambda p: exr.read_item(p, "host", "host"), paths))
            parts["read_host_pool"].append((time.perf_counter() - t0) * 1e3)
        parts["upload_batch"].append(wall(lambda: exr.upload_batch(items, dev)))
        data = np.concatenate([it.data for it in items])
        src_off = np.concatenate([[0]] + [it.src_offsets[1:] + o for it, o in zip(items, np.cumsum([0] + [it.data.size for it in items]))])
        dst_off = np.concatenate([[0]] + [it.offsets[1:] + o for it, o in zip(items, np.cumsum([0] + [int(it.offsets[-1]) for it in items]))])
        mode = torch.from_numpy(np.concatenate([it.mode for it in items])).to(dev)
        geom, words = [], []
        for it in items:
            h = it.header
            for c in range(h.n_chunks):
                geom.append((h.width, min(h.lines, h.height - c * h.lines), len(words), len(h.channels)))
            words += exr.piz_words(h)
        src = torch.from_numpy(data).to(dev)
        for s, (dec, wav) in stages.items():
            ms = []
            out = K.piz_decode(src, src_off, dst_off, np.asarray(geom, dtype=np.int32), words, mode=mode, sub_bits=s, stage_ms=ms, rounds=True)
            assert int(out[2].abs().sum()) == 0
            dec.append(ms[0])
            wav.append(ms[1])
            r = out[3][mode.bool()].cpu().numpy().astype(np.int64)
            rounds[s] = {int(k): int(v) for k, v in zip(*np.unique(r[:, 0], return_counts=True))}
            redone = r[:, 1:].sum(axis=0)                                # subsequences decoded in round 0, 1, ...: all, then the not yet final
            final[s] = [round(1.0 - float(redone[k + 1]) / float(redone[0]), 5) for k in range(redone.size - 1)]
    stored, decoded = int(src_off[-1]), int(dst_off[-1])
    return {"chunks": src_off.size - 1, "coded_chunks": int(mode.sum()), "stored_mb": round(stored / 1e6, 2), "decoded_mb": round(decoded / 1e6, 2),
            "parts_ms": {k: round(med(v), 3) for k, v in parts.items()},
            "stage_ms": {str(s): {"decode": round(med(d), 3), "wavelet": round(med(w), 3)} for s, (d, w) in stages.items()},
            "rounds_per_chunk": {str(s): r for s, r in rounds.items()},
            "share_final_after_round": {str(s): f for s, f in final.items()},
            "decoded_mb_per_s_default": round(decoded / 1e6 / ((med(stages[K.PIZ_SUB_BITS][0]) + med(stages[K.PIZ_SUB_BITS][1])) / 1e3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--compression", choices=("zip", "zips", "piz"), default="zip")
    ap.add_argument("--inflate", choices=("host", "device", "both"), default="host")
    ap.add_argument("--piz", choices=("host", "device", "both"), default="host")
    ap.add_argument("--out")
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    is_piz = a.compression == "piz"
    choice = a.piz if is_piz else a.inflate
    routes = ("host", "device") if choice == "both" else (choice,)
    option = "exr_piz" if is_piz else "exr_inflate"
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        img = _image(rng, a.height, a.width)
        names = []
        for i in range(a.files):
            ch = {c: (img * (1.0 + 0.1 * k + 0.01 * i), X.HALF) for k, c in enumerate("RGB")}
            ch["A"] = (np.ones_like(img), X.HALF)
            name = "f%03d.exr" % i
            if not is_piz:
                X.write_exr(os.path.join(d, name), ch, X.ZIP if a.compression == "zip" else X.ZIPS)
            elif i == 0:
                piz_ref.write_exr(os.path.join(d, name), ch, fast=True)
            else:
                with open(os.path.join(d, names[0]), "rb") as f0, open(os.path.join(d, name), "wb") as f1:
                    f1.write(f0.read())
            names.append(name)
        mb = sum(os.path.getsize(os.path.join(d, n)) for n in names) / 1e6
        write_s = time.perf_counter() - t0
        runs = {r: [] for r in routes}
        arenas = {}
        for r in routes:                                                  # warm-up (and the arenas to compare), not timed
            arenas[r] = dataset.PatchHDRDataset(d, names, True, **{option: r}).arena
        if len(routes) == 2:
            assert torch.equal(arenas["host"].view(torch.int32), arenas["device"].view(torch.int32)), "the two routes' arenas differ"
        arenas.clear()
        for _ in range(a.repeat):                                         # alternating windows
            for r in routes:
                ds = dataset.PatchHDRDataset(d, names, True, **{option: r})
                runs[r].append(ds.load_seconds)
                del ds
        result = {"files": a.files, "width": a.width, "height": a.height, "compression": a.compression.upper(), "file_mb": round(mb, 1),
                  "write_s": round(write_s, 2)}
        first = routes[0]
        host = float(np.median([r["host_decode"] for r in runs[first]]))
        dev = float(np.median([r["device"] for r in runs[first]]))
        result.update({"piz" if is_piz else "inflate": choice, "host_decode_s": round(host, 4), "device_s": round(dev, 4),
                       "device_share": round(dev / (host + dev), 3), "host_runs": [round(r["host_decode"], 4) for r in runs[first]],
                       "device_runs": [round(r["device"], 4) for r in runs[first]]})
        if len(routes) == 2:
            for r in routes:
                h = float(np.median([x["host_decode"] for x in runs[r]]))
                v = float(np.median([x["device"] for x in runs[r]]))
                result[r + "_route"] = {"host_decode_s": round(h, 4), "device_s": round(v, 4), "load_s": round(h + v, 4),
                                        "load_runs": [round(x["host_decode"] + x["device"], 4) for x in runs[r]]}
            result["device_over_host"] = round(result["device_route"]["load_s"] / result["host_route"]["load_s"], 3)
            result["device_route_parts"] = (piz_device_parts if is_piz else device_parts)([os.path.join(d, n) for n in names], a.repeat)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

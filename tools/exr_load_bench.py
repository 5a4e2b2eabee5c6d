"""Load time of the training-set reader on OpenEXR files: writes N synthetic ZIP files (HALF R, G, B, A; 3840 x 2160 by
default) to a temporary directory, builds PatchHDRDataset over them and prints its load_seconds (host decode: read + inflate in
the thread pool; device: upload, unpredict, load-resize, means), the median of --repeat builds, as one JSON line.

    python tools/exr_load_bench.py [--files 8] [--width 3840] [--height 2160] [--repeat 3]
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import exr_ref as X  # noqa: E402

pkg = importlib.import_module("singlehdr-tf2_amd")


def _image(rng, h, w):
    """smooth gradients plus a little noise: compresses about as well as a rendered HDR frame"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = np.exp(2.0 * np.sin(x / 300.0) * np.cos(y / 200.0))
    return (base * (1.0 + 0.02 * rng.standard_normal((h, w)).astype(np.float32))).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        img = _image(rng, a.height, a.width)
        names = []
        for i in range(a.files):
            ch = {c: (img * (1.0 + 0.1 * k + 0.01 * i), X.HALF) for k, c in enumerate("RGB")}
            ch["A"] = (np.ones_like(img), X.HALF)
            name = "f%03d.exr" % i
            X.write_exr(os.path.join(d, name), ch, X.ZIP)
            names.append(name)
        mb = sum(os.path.getsize(os.path.join(d, n)) for n in names) / 1e6
        write_s = time.perf_counter() - t0
        runs = []
        for _ in range(a.repeat):
            ds = pkg.dataset.PatchHDRDataset(d, names, True)
            runs.append(ds.load_seconds)
            del ds
        host = float(np.median([r["host_decode"] for r in runs]))
        dev = float(np.median([r["device"] for r in runs]))
    print(json.dumps({"files": a.files, "width": a.width, "height": a.height, "compression": "ZIP", "file_mb": round(mb, 1),
                      "write_s": round(write_s, 2), "host_decode_s": round(host, 4), "device_s": round(dev, 4),
                      "device_share": round(dev / (host + dev), 3), "host_runs": [round(r["host_decode"], 4) for r in runs],
                      "device_runs": [round(r["device"], 4) for r in runs]}))


if __name__ == "__main__":
    main()

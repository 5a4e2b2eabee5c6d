"""Score a checkpoint: PSNR-L, PSNR-mu, SSIM-mu and the fine-tuning loss of the four nets on validation pairs, one JSON line per
precision -- "fp16 costs X dB PSNR-mu" as a command.

    python tools/evaluate.py --checkpoints CKPT_DIR --data HDR_REAL_DIR [--precisions fp32,fp16] [--batch-size 8]
    python tools/evaluate.py --synthetic [--pairs 4] [--side 512]          # seeded nets and a synthetic folder: a dry run

CKPT_DIR holds the reference's four CheckpointManager directories deq/, lin/, hal/, ref/ (tf_checkpoint.restore); HDR_REAL_DIR
holds HDR_gt/*.hdr|*.exr and LDR_in/*.jpg (hdr_real.HdrRealFolder, read with augment=False: every kept 256 x 256 patch once).
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pkg = importlib.import_module("singlehdr-tf2_amd")
NETS = dict(deq="dequantization_net", lin="linearization_net", hal="hallucination_net", ref="refinement_net")


def synthetic_pair(rng, side):
    """a smooth scene of a few stops with noise, and its clipped 8-bit rendering"""
    y, x = np.mgrid[0:side, 0:side].astype(np.float32) / side
    base = 0.5 + 0.3 * np.sin(6.0 * x + rng.random() * 6.0) * np.cos(5.0 * y + rng.random() * 6.0)
    hdr = (np.exp2(4.0 * base[..., None]) * (1.0 + 0.05 * rng.standard_normal((side, side, 3)))).astype(np.float32)
    ldr = np.clip(255.0 * (hdr / 8.0) ** (1 / 2.2), 0, 255).astype(np.uint8)
    return ldr, hdr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--checkpoints")
    ap.add_argument("--data")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--side", type=int, default=512)
    ap.add_argument("--precisions", default="fp32,fp16")
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--no-normalise", action="store_true", help="compare absolute values instead of mean-normalised images")
    a = ap.parse_args()
    if not a.synthetic and not (a.checkpoints and a.data):
        ap.error("give --checkpoints and --data, or --synthetic")
    if not torch.cuda.is_available():
        raise SystemExit("evaluate.py needs a HIP device (there is no CPU fallback)")
    models = {}
    for i, (k, mod) in enumerate(NETS.items()):
        models[k] = getattr(pkg, mod).model()
        if a.checkpoints:
            pkg.tf_checkpoint.restore(models[k], os.path.join(a.checkpoints, k))
        else:
            from oracle import nets
            models[k].load_numpy(nets.init_params(getattr(nets, k + "_spec")(), 100 + i))
    if a.data:
        folder = pkg.hdr_real.HdrRealFolder(a.data, batch_size=a.batch_size, augment=False)
    else:
        rng = np.random.default_rng(0)
        ldr, hdr = zip(*[synthetic_pair(rng, a.side) for _ in range(a.pairs)])
        folder = pkg.hdr_real.HdrRealFolder.from_arrays(ldr, hdr, batch_size=a.batch_size, augment=False)
    for precision in a.precisions.split(","):
        run = pkg.pipeline.Inference(models["deq"], models["lin"], models["hal"], models["ref"], precision=precision)
        ev = pkg.pipeline.Evaluate(run, pkg.metrics.Evaluator(normalise=not a.no_normalise))
        out = {"precision": precision, "patches": len(folder.patches)}
        out.update({k: (round(v, 6) if isinstance(v, float) else v) for k, v in ev.run(iter(folder)).items()})
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

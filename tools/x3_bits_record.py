"""Record tests/golden/x3_prefetch_bits.json: for every run of tests/test_gpu_x3_prefetch.py (`entries()`), the SHA-256 of every input
tensor and the SHA-256 and shape of every output -- y, pooled, projected, range slot, dx.

    python tools/x3_bits_record.py --commit <the commit the library was built from> [--out FILE]

The recorded library is the one the package loads (SHDR_LIB names another build) under the switches of the environment; the committed
file was written from the last commit that had the load order of the first rounds, with SHDR_X3_LEGACY_PREFETCH=1.  Record again only
when a change alters the summation order of conv_x3_kernel on purpose: the tests then compare with what this tool saw."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ["SHDR_X3_MIN_BLOCKS"] = "1"                        # as the tests set it (read by the library when it loads)

import torch  # noqa: E402

import test_gpu_x3_prefetch as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="commit of the library that is recorded")
    ap.add_argument("--out", default=T.GOLDEN)
    args = ap.parse_args()
    K = importlib.import_module("singlehdr-tf2_amd")._ops
    switches = {k: v for k, v in sorted(os.environ.items()) if k.startswith("SHDR_X3_")}
    runs = {}
    for key, build in T.entries(K).items():
        tensors, run, names = build()
        with torch.no_grad():
            out = run()
        torch.cuda.synchronize()
        assert len(out) == len(names), key
        runs[key] = dict(inputs=[T.digest(t) for t in tensors if t is not None],
                         outputs=[dict(name=n, shape=list(t.shape), sha256=T.digest(t)) for n, t in zip(names, out)])
        print(key, [o["sha256"][:8] for o in runs[key]["outputs"]], flush=True)
    with open(args.out, "w") as f:
        json.dump(dict(commit=args.commit, switches=switches, torch=torch.__version__, runs=runs), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out, len(runs), "runs")


if __name__ == "__main__":
    main()

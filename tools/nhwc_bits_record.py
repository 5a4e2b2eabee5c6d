"""Record tests/golden/nhwc_family_bits.json: for every run of tests/test_gpu_nhwc_bits.py (`entries()`), the SHA-256 of every input
tensor and the SHA-256 and shape of every output.

    python tools/nhwc_bits_record.py --commit <the commit the library was built from> [--out FILE] [--same-as FILE]

The recorded library is the one the package loads (SHDR_LIB names another build).  --same-as compares the digests with an earlier
recording and fails on the first run that differs: an output that is not stable between two recordings does not belong in the file.
Record again only when a change alters the arithmetic of the NHWC pooling / resize kernels or the BatchNorm finalisers on purpose: the
test then compares with what this tool saw."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

import test_gpu_nhwc_bits as T  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="commit of the library that is recorded")
    ap.add_argument("--out", default=T.GOLDEN)
    ap.add_argument("--same-as", default=None, help="an earlier recording that this one has to reproduce")
    args = ap.parse_args()
    K = importlib.import_module("singlehdr-tf2_amd")._ops
    runs = {}
    for key, build in sorted(T.entries(K).items()):
        tensors, run, names = build()
        with torch.no_grad():
            out = run()
        torch.cuda.synchronize()
        assert len(out) == len(names), key
        runs[key] = dict(inputs=[T.digest(t) for t in tensors],
                         outputs=[dict(name=n, shape=list(t.shape), sha256=T.digest(t)) for n, t in zip(names, out)])
        print(key, [o["sha256"][:8] for o in runs[key]["outputs"]], flush=True)
    if args.same_as:
        with open(args.same_as) as f:
            before = json.load(f)["runs"]
        unstable = [k for k in sorted(runs) if runs[k] != before.get(k)]
        assert not unstable, "not the digests of %s: %s" % (args.same_as, unstable)
    with open(args.out, "w") as f:
        json.dump(dict(commit=args.commit, torch=torch.__version__, runs=runs), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out, len(runs), "runs")


if __name__ == "__main__":
    main()

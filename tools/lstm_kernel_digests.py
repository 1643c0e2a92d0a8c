#!/usr/bin/env python3
"""sha256 of what the recurrent inference kernels write, per case of tests/lstm_digests.py: tests/golden/lstm_kernels_parent.json.

    python tools/lstm_kernel_digests.py LIBRARY [--out FILE]

LIBRARY is the libbonito_hip.so to pin, loaded in place of the tree's own. The committed file was written once on an MI355X against a build
of the commit BEFORE the kernels of csrc/lstm.hip and csrc/lstm_q8.hip moved their shared parts into csrc/lstm_ring.h;
tests/test_gpu_lstm.py and tests/test_gpu_q8.py recompute the digests with the tree's library and compare. Cases, inputs and the entries
(bh_lstm_layer_family, bh_lstm_q8_layer, and the engine for the "lstm_tune" bits) are those of tests/lstm_digests.py. The kernels have no
atomics in their arithmetic and no order that depends on scheduling, so the bytes do not depend on the machine."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("library")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lstm_kernels_parent.json"))
    args = ap.parse_args()
    os.environ["BONITO_HIP_LIB"] = os.path.abspath(args.library)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    import lstm_digests as ld
    if not torch.cuda.is_available():
        raise SystemExit("lstm_kernel_digests: no HIP device")
    doc = {"seed": ld.SEED,
           "fp16": {f: {ld.fp16_key(*c): ld.fp16_digest(f, *c) for c in ld.fp16_cases(f)} for f in ld.WIDTHS},
           "q8": {ld.q8_key(*c): ld.q8_digest(*c) for c in ld.q8_cases()},
           "engine": {name: ld.engine_digest(name) for name in ld.ENGINE_CASES}}
    with open(args.out, "w") as fh:
        fh.write(json.dumps(doc, indent=1) + "\n")
    print("%s: %d fp16, %d q8, %d engine cases" % (args.out, sum(len(v) for v in doc["fp16"].values()), len(doc["q8"]), len(doc["engine"])))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time the Smith-Waterman aligner (bonito_amd/csrc/align.hip, bh_sw_align) on the two shapes that matter: the chunks of an
`evaluate` run (512 pairs at about 800 bases, what a 10 000-sample chunk calls) and the largest supported pairs (64 at 4096).

    python tools/align_bench.py [--iters 20 --warmup 3 --error-rate 0.1 --out FILE]

Each reference is seeded random; its query is a copy with about 10 % planted errors (substitutions, insertions, deletions in equal
shares), cut to the supported length. HIP events on the current stream around `iters` back-to-back calls of the C entry after
`warmup` calls, the code planes already on the device; a call = the copy of the lengths, the forward kernel (4 traceback bits per
cell) and the traceback kernel. Reported per shape: milliseconds and cell updates per second (sum of seq_len x ref_len over the
pairs, per call), with and without the run-length CIGAR output. Prints one JSON object (and writes it to --out).
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bonito_amd import _lib  # noqa: E402
from bonito_amd.align import MAX_LEN  # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def make_pairs(rng, n, length, rate):
    """-> code planes int8 [n, L] (1..4, 0 padding) and int32 lengths for refs and their mutated copies."""
    refs = rng.integers(1, 5, size=(n, length)).astype(np.int8)
    seqs = np.zeros((n, MAX_LEN), np.int8)
    lens = np.zeros(n, np.int32)
    for i in range(n):
        u = rng.random(length)
        sub = u < rate / 3
        row = np.where(sub, (refs[i] - 1 + rng.integers(1, 4, size=length)) % 4 + 1, refs[i]).astype(np.int8)
        keep = ~((u >= 2 * rate / 3) & (u < rate))                          # deletions
        ins = (u >= rate / 3) & (u < 2 * rate / 3)                          # a random base after these
        out = np.stack([row, np.where(ins, rng.integers(1, 5, size=length), 0).astype(np.int8)], axis=1)
        out[~keep, 0] = 0
        flat = out.reshape(-1)
        flat = flat[flat != 0][:MAX_LEN]
        seqs[i, :len(flat)] = flat
        lens[i] = len(flat)
    width = int(lens.max())
    return seqs[:, :width].copy(), lens, refs, np.full(n, length, np.int32)


def bench_shape(lib, dev, rng, n, length, rate, iters, warmup):
    seqs, sl, refs, rl = make_pairs(rng, n, length, rate)
    s_dev, r_dev = torch.from_numpy(seqs).to(dev), torch.from_numpy(refs).to(dev)
    ms, mr = int(sl.max()), int(rl.max())
    nbytes = lib.bh_sw_workspace(n, ms, mr)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    res = torch.empty((n, 10), dtype=torch.int32, device=dev)
    stride = ms + mr - 1
    ops = torch.empty((n, stride), dtype=torch.int32, device=dev)
    n_ops = torch.empty(n, dtype=torch.int32, device=dev)
    ip = C.POINTER(C.c_int32)
    st = _lib.stream_ptr(dev)

    def call(with_ops):
        _lib.check(lib.bh_sw_align(_lib.ptr(s_dev), s_dev.shape[1], sl.ctypes.data_as(ip), _lib.ptr(r_dev), r_dev.shape[1],
                                   rl.ctypes.data_as(ip), n, 5, -4, 8, 4, _lib.ptr(ws), nbytes, _lib.ptr(res),
                                   _lib.ptr(ops) if with_ops else None, stride if with_ops else 0,
                                   _lib.ptr(n_ops) if with_ops else None, st), "bh_sw_align")

    ms_plain = timed(lambda: call(False), iters, warmup)
    ms_cigar = timed(lambda: call(True), iters, warmup)
    table = res.cpu().numpy().astype(np.int64)
    cells = int((sl.astype(np.int64) * rl.astype(np.int64)).sum())
    total = table[:, 1:5].sum(axis=1)
    return {
        "pairs": n, "ref_len": length, "mean_seq_len": float(sl.mean()), "cells_per_call": cells,
        "workspace_bytes": int(nbytes),
        "ms": ms_plain, "ms_with_cigar": ms_cigar,
        "cell_updates_per_second": cells / (ms_plain * 1e-3), "cell_updates_per_second_with_cigar": cells / (ms_cigar * 1e-3),
        "mean_accuracy": float((table[:, 1] / np.maximum(total, 1)).mean()), "mean_cigar_runs": float(n_ops.cpu().numpy().mean()),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--error-rate", type=float, default=0.1)
    ap.add_argument("--out")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    rng = np.random.default_rng(25)
    res = {
        "chunks_512x800": bench_shape(lib, dev, rng, 512, 800, args.error_rate, args.iters, args.warmup),
        "largest_64x4096": bench_shape(lib, dev, rng, 64, MAX_LEN, args.error_rate, args.iters, args.warmup),
        "scoring": {"match": 5, "mismatch": -4, "gap_open": 8, "gap_extend": 4}, "error_rate": args.error_rate,
        "iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
    }
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time the banded global aligner (bonito_amd/csrc/nw.hip through align.nw_align) on the two shapes of a duplex run: 512 pairs of
about 10 000 bases and 64 pairs of about 50 000 bases, both at about 5 % divergence.

    python tools/duplex_bench.py [--iters 3 --warmup 1 --error-rate 0.05 --band 64 --out profiles/duplex_bench.json]

Each reference is seeded random; its query is a copy with planted errors (substitutions, insertions, deletions in equal shares).
Wall time around whole `nw_align` calls with the run-length ops, from code planes on the host to results on the host: every band
round (a rejected pair runs again with the half-width doubled), the slicing by the workspace budget, the copies and the traceback
are inside. Reported per shape: milliseconds, pairs per second, band cells per second (sum over the pairs of seq_len x the width of the
accepted band, per call - the cells of the rejected rounds are work too, but not counted), the share of pairs that needed a second
band and the accepted half-widths. Prints one JSON object (and writes it to --out).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bonito_amd.align import nw_align  # noqa: E402


def make_pairs(rng, n, length, rate):
    """-> code planes int8 [n, L] (1..4, 0 padding) for the mutated copies and their references"""
    refs = rng.integers(1, 5, size=(n, length)).astype(np.int8)
    rows = []
    for i in range(n):
        u = rng.random(length)
        row = np.where(u < rate / 3, (refs[i] - 1 + rng.integers(1, 4, size=length)) % 4 + 1, refs[i]).astype(np.int8)
        ins = (u >= rate / 3) & (u < 2 * rate / 3)                          # a random base after these
        out = np.stack([row, np.where(ins, rng.integers(1, 5, size=length), 0).astype(np.int8)], axis=1)
        out[(u >= 2 * rate / 3) & (u < rate), 0] = 0                        # deletions
        flat = out.reshape(-1)
        rows.append(flat[flat != 0])
    seqs = np.zeros((n, max(len(r) for r in rows)), np.int8)
    for i, r in enumerate(rows):
        seqs[i, :len(r)] = r
    return seqs, refs


def bench_shape(rng, n, length, rate, band, iters, warmup):
    seqs, refs = make_pairs(rng, n, length, rate)
    got = None
    for _ in range(warmup):
        got = nw_align(seqs, refs, band=band)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        got = nw_align(seqs, refs, band=band)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / iters * 1e3
    assert (got.status == 0).all()
    sl, rl, k = got.seq_len.astype(np.int64), got.ref_len.astype(np.int64), got.band.astype(np.int64)
    cells = int((sl * np.minimum(rl, np.abs(rl - sl) + 2 * k + 1)).sum())
    table = got.table.astype(np.int64)
    return {
        "pairs": n, "ref_len": length, "mean_seq_len": float(sl.mean()), "first_band": band,
        "ms": ms, "pairs_per_second": n / (ms * 1e-3), "band_cells_per_call": cells, "band_cells_per_second": cells / (ms * 1e-3),
        "share_needing_a_second_band": float((k > band).mean()),
        "accepted_bands": {str(v): int((k == v).sum()) for v in sorted(set(k.tolist()))},
        "mean_distance": float(table[:, 0].mean()), "mean_cigar_runs": float(table[:, 5].mean()),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--error-rate", type=float, default=0.05)
    ap.add_argument("--band", type=int, default=64, help="the first half-width")
    ap.add_argument("--out")
    args = ap.parse_args()
    rng = np.random.default_rng(26)
    res = {
        "reads_512x10000": bench_shape(rng, 512, 10000, args.error_rate, args.band, args.iters, args.warmup),
        "long_64x50000": bench_shape(rng, 64, 50000, args.error_rate, args.band, args.iters, args.warmup),
        "error_rate": args.error_rate, "iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
    }
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

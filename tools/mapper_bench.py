#!/usr/bin/env python3
"""Time the device read mapper (bonito_amd/aligner.py: csrc/mapper.hip for sketch / seed / chain, csrc/nw.hip for the bases) on the
two shapes of a basecalling run with --reference: 512 reads of about 10 000 bases and 64 reads of about 50 000 bases, planted at
about 5 % divergence on both strands of a seeded random reference of 5 Mb.

    python tools/mapper_bench.py [--iters 3 --warmup 1 --error-rate 0.05 --ref-len 5000000 --out profiles/mapper_bench.json]

Wall time around whole `Aligner.map_batch` calls, from strings on the host to `Mapping` records on the host. Reported per shape:
milliseconds per call, split into sketch + seed (+ the sort of the anchors), chain (+ the prefix sums and the copy of its results),
base alignment (`align.nw_align` over all pieces: every band round, copies and traceback) and host assembly (spans and pieces before
it; CIGAR merge, NM and MD after it), reads and bases per second, the share of reads mapped to the place they were cut from, and the
time to build the index. Prints one JSON object (and writes it to --out).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bonito_amd.aligner import Aligner  # noqa: E402

LETTERS = np.frombuffer(b"ACGT", np.uint8)
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def planted_reads(rng, ref, n, length, rate):
    """-> [(read, true start, true end, strand)]: copies with substitutions, insertions and deletions in equal shares"""
    out = []
    for _ in range(n):
        start = int(rng.integers(0, len(ref) - length))
        src = ref[start:start + length]
        u = rng.random(length)
        row = np.where(u < rate / 3, (src + rng.integers(1, 4, size=length)) % 4, src).astype(np.int8)
        ins = (u >= rate / 3) & (u < 2 * rate / 3)                          # a random base after these
        two = np.stack([row, np.where(ins, rng.integers(0, 4, size=length), -1).astype(np.int8)], axis=1)
        two[(u >= 2 * rate / 3) & (u < rate), 0] = -1                       # deletions
        flat = two.reshape(-1)
        read = LETTERS[flat[flat >= 0]].tobytes()
        strand = 1 if rng.random() < 0.5 else -1
        out.append(((read if strand == 1 else read.translate(COMP)[::-1]).decode(), start, start + length, strand))
    return out


def bench_shape(aligner, reads, iters, warmup):
    seqs = [r[0] for r in reads]
    got = None
    for _ in range(warmup):
        got = aligner.map_batch(seqs)
    for key in aligner.timings:
        aligner.timings[key] = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        got = aligner.map_batch(seqs)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / iters * 1e3
    right = sum(m is not None and m.strand == s and st - 50 <= m.r_st and m.r_en <= en + 50 for m, (_, st, en, s) in zip(got, reads))
    bases = sum(len(s) for s in seqs)
    split = {name: sec / iters * 1e3 for name, sec in aligner.timings.items()}
    return {
        "reads": len(seqs), "mean_read_len": bases / len(seqs), "ms": ms, "ms_sketch_seed": split["sketch_seed"], "ms_chain": split["chain"],
        "ms_base_alignment": split["base"], "ms_host_assembly": split["host"], "host_assembly_share": split["host"] / ms,
        "reads_per_second": len(seqs) / (ms * 1e-3), "bases_per_second": bases / (ms * 1e-3),
        "mapped": sum(m is not None for m in got), "mapped_in_place": right,
        "mean_identity": float(np.mean([m.mlen / m.blen for m in got if m is not None])) if any(m is not None for m in got) else 0.0,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--error-rate", type=float, default=0.05)
    ap.add_argument("--ref-len", type=int, default=5000000)
    ap.add_argument("--out")
    args = ap.parse_args()
    rng = np.random.default_rng(27)
    ref = rng.integers(0, 4, size=args.ref_len).astype(np.int8)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    aligner = Aligner([("ref", LETTERS[ref].tobytes().decode())])
    torch.cuda.synchronize()
    index_ms = (time.perf_counter() - t0) * 1e3
    res = {
        "reads_512x10000": bench_shape(aligner, planted_reads(rng, ref, 512, 10000, args.error_rate), args.iters, args.warmup),
        "long_64x50000": bench_shape(aligner, planted_reads(rng, ref, 64, 50000, args.error_rate), args.iters, args.warmup),
        "index_ms": index_ms, "index_minimizers": int(aligner.index_keys.numel()), "ref_len": args.ref_len, "k": aligner.k, "w": aligner.w,
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

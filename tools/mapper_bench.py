#!/usr/bin/env python3
"""Time the device read mapper (bonito_amd/aligner.py: csrc/mapper.hip for sketch / seed / chain, csrc/nw.hip for the bases) on the
two shapes of a basecalling run with --reference: 512 reads of about 10 000 bases and 64 reads of about 50 000 bases, planted at
about 5 % divergence on both strands of a seeded random reference of 5 Mb.

    python tools/mapper_bench.py [--iters 3 --warmup 1 --error-rate 0.05 --ref-len 5000000 --out profiles/mapper_bench.json]
    python tools/mapper_bench.py --extend-ends --out profiles/mapper_extend_bench.json

Wall time around whole `Aligner.map_batch` calls, from strings on the host to `Mapping` records on the host. Reported per shape:
milliseconds per call, split into sketch + seed (+ the sort of the anchors), chain (+ the prefix sums and the copy of its results),
base alignment (`align.nw_align` over all pieces: every band round, copies and traceback) and host assembly (spans and pieces before
it; CIGAR merge, NM and MD after it), reads and bases per second, the share of reads mapped to the place they were cut from, and the
time to build the index. Prints one JSON object (and writes it to --out).

With --extend-ends every shape is timed in the same process without and with the end extension (`bh_map_extend`, one launch
per `map_batch` call for both ends of every mapping): the entry of a shape then holds the run without it under "plain" (and once more,
after the other, under "plain_again"), the run with it under "extended" (its table has the additional stage "ms_extend"), and in
all of them the share of reads whose alignment reaches both ends of the read.
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


def bench_shape(aligner, reads, iters, warmup, extend=None):
    """extend: None = the tool's standing table; False / True = the same with `extend_ends` passed, the extension's stage and the
    share of reads aligned from their first to their last base"""
    seqs = [r[0] for r in reads]
    got = None
    kw = {} if extend is None else {"extend_ends": extend}
    for _ in range(warmup):
        got = aligner.map_batch(seqs, **kw)
    for key in aligner.timings:
        aligner.timings[key] = 0.0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        got = aligner.map_batch(seqs, **kw)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / iters * 1e3
    right = sum(m is not None and m.strand == s and st - 50 <= m.r_st and m.r_en <= en + 50 for m, (_, st, en, s) in zip(got, reads))
    bases = sum(len(s) for s in seqs)
    split = {name: sec / iters * 1e3 for name, sec in aligner.timings.items()}
    more = {} if extend is None else {
        "ms_extend": split["extend"],
        "both_ends_reached": sum(m is not None and m.q_st == 0 and m.q_en == len(s) for m, s in zip(got, seqs)) / len(seqs)}
    return {
        **more,
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
    ap.add_argument("--extend-ends", action="store_true", help="time every shape without and with the end extension")
    ap.add_argument("--out")
    args = ap.parse_args()
    rng = np.random.default_rng(27)
    ref = rng.integers(0, 4, size=args.ref_len).astype(np.int8)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    aligner = Aligner([("ref", LETTERS[ref].tobytes().decode())])
    torch.cuda.synchronize()
    index_ms = (time.perf_counter() - t0) * 1e3
    def shape(reads):
        if not args.extend_ends:
            return bench_shape(aligner, reads, args.iters, args.warmup)
        # the run without the option twice, before and after: what the two differ by is what the box does between runs of one code path
        return {"plain": bench_shape(aligner, reads, args.iters, args.warmup, extend=False),
                "extended": bench_shape(aligner, reads, args.iters, args.warmup, extend=True),
                "plain_again": bench_shape(aligner, reads, args.iters, args.warmup, extend=False)}

    res = {
        "reads_512x10000": shape(planted_reads(rng, ref, 512, 10000, args.error_rate)),
        "long_64x50000": shape(planted_reads(rng, ref, 64, 50000, args.error_rate)),
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

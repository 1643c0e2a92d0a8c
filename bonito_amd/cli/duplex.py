"""
``python -m bonito_amd duplex <calls> <pairs_file> > duplex.fastq``: basespace duplex calling of (template, complement) read pairs
(the reference's ``bonito duplex``, bonito/cli/duplex.py:325-397, with its DuplexWriter, bonito/io.py:472-502). The alignments run on
the device (bonito_amd/duplex.py); there is no --reference, this build has no mapper.
"""
import sys
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser
from datetime import timedelta
from time import perf_counter

import numpy as np

from bonito_amd import duplex
from bonito_amd.io import write_fastq
from bonito_amd.util import mean_qscore_from_qstring


def read_calls(path):
    """A FASTQ or an unaligned SAM as the basecaller writes them -> {read id: (sequence, quality string)}. A read's id is its first
    token; on a duplicated id the first record counts."""
    calls = {}
    with open(path) as fh:
        first = fh.readline()
        if not first:
            return calls
        if first[:3] in ("@HD", "@SQ", "@RG", "@PG", "@CO") and first[3:4] == "\t":                      # a SAM header line
            sam = True
        else:
            sam = "\t" in first and not first.startswith("@") and len(first.split("\t")) >= 11
        fh.seek(0)
        if sam:
            for line in fh:
                if line.startswith("@") or not line.strip():
                    continue
                f = line.rstrip("\n").split("\t")
                if len(f) < 11:
                    raise ValueError("%s: a SAM record with %d fields" % (path, len(f)))
                if int(f[1]) & 0x900:                                                 # secondary / supplementary
                    continue
                seq, qual = f[9], f[10]
                if seq == "*":
                    seq = ""
                if qual == "*" and len(seq) != 1:
                    qual = "!" * len(seq)
                calls.setdefault(f[0].split()[0], (seq, qual))
        else:
            while True:
                head = fh.readline()
                if not head:
                    break
                if not head.strip():
                    continue
                seq, plus, qual = fh.readline().rstrip("\n"), fh.readline(), fh.readline().rstrip("\n")
                if not head.startswith("@") or not plus.startswith("+") or len(seq) != len(qual):
                    raise ValueError("%s: not a four-line FASTQ record at %r" % (path, head.strip()[:60]))
                calls.setdefault(head[1:].split()[0], (seq, qual))
    return calls


def read_pairs(path, header=True):
    """template id and complement id per line, separated by whitespace; the first line is a header unless told otherwise"""
    pairs = []
    with open(path) as fh:
        if header:
            fh.readline()
        for line in fh:
            if not line.strip():
                continue
            temp, comp = line.split()[:2]
            pairs.append((temp, comp))
    return pairs


def call(pairs, calls, batch=512, device="cuda", stats=None):
    """-> one (sequence, quality string) per pair, in order; ("", "") for a pair with a missing read"""
    out = [("", "")] * len(pairs)
    known = [i for i, (t, c) in enumerate(pairs) if t in calls and c in calls]
    if stats is not None:
        stats["missing"] = stats.get("missing", 0) + len(pairs) - len(known)
    for lo in range(0, len(known), batch):
        idx = known[lo:lo + batch]
        temp, comp = [calls[pairs[i][0]] for i in idx], [calls[pairs[i][1]] for i in idx]
        got = duplex.call_pairs([t[0] for t in temp], [t[1] for t in temp], [c[0] for c in comp], [c[1] for c in comp],
                                device=device, stats=stats)
        for i, res in zip(idx, got):
            out[i] = res
    return out


def main(args):
    sys.stderr.write("> outputting unaligned fastq\n")
    calls = read_calls(args.calls)
    pairs = read_pairs(args.duplex_pairs_file, header=not args.no_header)
    stats = {}
    t0 = perf_counter()
    results = call(pairs, calls, batch=args.batch, device=args.device, stats=stats)
    log = []
    for (temp, comp), (seq, qstring) in zip(pairs, results):
        read_id = "%s;%s" % (temp, comp)
        mean_q = mean_qscore_from_qstring(qstring) if len(qstring) else 0.0
        log.append((read_id, len(seq)))
        if mean_q < args.min_qscore or not len(seq):
            continue
        write_fastq(read_id, seq, qstring, fd=sys.stdout, tags=["qs:i:%d" % round(mean_q)])
    sys.stdout.flush()
    duration = perf_counter() - t0
    duplex.report(stats)
    if stats.get("missing"):
        sys.stderr.write("> pairs with a missing read: %d\n" % stats["missing"])
    sys.stderr.write("> empty calls: %d\n" % sum(1 for _, n in log if n == 0))
    sys.stderr.write("> completed reads: %s\n" % len(log))
    sys.stderr.write("> duration: %s\n" % timedelta(seconds=np.round(duration)))
    sys.stderr.write("> bases per second %.1E\n" % (sum(n for _, n in log) / max(duration, 1e-9)))
    sys.stderr.write("> done\n")
    return 0


def argparser():
    parser = ArgumentParser(
        formatter_class=ArgumentDefaultsHelpFormatter,
        add_help=False,
        description="Basespace duplex calling: the consensus of template / complement read pairs, aligned on the device, as FASTQ on "
                    "stdout. <calls> is a FASTQ or an unaligned SAM as `bonito_amd basecaller` writes them (BAM needs pysam, which "
                    "this build does not have); there is no --reference (no mapper).",
    )
    parser.add_argument("calls")
    parser.add_argument("duplex_pairs_file")
    parser.add_argument("--min-qscore", default=0, type=int)
    parser.add_argument("--no-header", action="store_true")
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--batch", default=512, type=int, help="pairs per alignment batch")
    return parser

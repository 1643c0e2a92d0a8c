"""
Basespace duplex calling, batched: the engine's counterpart of the reference's ``call_basespace_duplex`` and what it calls
(bonito/cli/duplex.py:109-300). The two alignments run on the device - one ``align.nw_align`` batch over all pairs (edlib's part) and
two ``align.sg_align`` batches for the read ends (parasail's part) - and everything that is O(length) stays on the host in numpy,
in the reference's dtypes. The definitions are in DESIGN.md section 6. There is no host fallback for the alignments.
"""
import re
import sys

import numpy as np

from bonito_amd import align as al

NUM_MATCH = 11                                   # an '=' run of this length anchors the end repair and the trim
GAP = ord("-")
_COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
_RUN = re.compile(r"(\d+)([=XID])")
_HOMOPOLYMER = re.compile(rb"(.)\1+", re.S)


def revcomp(seq):
    return seq.encode("ascii")[::-1].translate(_COMPLEMENT).decode("ascii")


def adjust_qscores(qscores, seq, qshift, pool=5):
    """Phred scores (uint8) of one read -> float32: shifted by ``qshift`` positions with the edge value repeated, an edge-padded
    minimum over ``pool`` positions, then the mean over every homopolymer run of two or more bases (reference: adj_qscores)."""
    q = np.asarray(qscores)
    n = len(q)
    if n == 0:
        return np.zeros(0, np.float32)
    q = q[np.clip(np.arange(n) - qshift, 0, n - 1)].astype(np.float32)
    padded = np.pad(q, pool // 2, mode="edge")
    q = np.lib.stride_tricks.sliding_window_view(padded, pool).min(axis=1)
    spans = [m.span() for m in _HOMOPOLYMER.finditer(seq.encode("ascii"))]
    if spans:
        st, en = np.array(spans).T
        size = en - st
        # the scores are whole numbers: their sum is exact in any order, and one float32 division rounds as the float32 mean does
        total = np.concatenate([[0.0], np.cumsum(q, dtype=np.float64)])
        mean = (total[en] - total[st]).astype(np.float32) / size.astype(np.float32)
        q[np.repeat(st - (np.cumsum(size) - size), size) + np.arange(size.sum())] = np.repeat(mean, size)
    return q


def parse_cigar(cigar):
    """'3=1X' -> [(3, '='), (1, 'X')]"""
    return [(int(k), c) for k, c in _RUN.findall(cigar)]


def lengths(ops):
    """-> (query bases, reference bases) the runs consume"""
    return sum(k for k, c in ops if c != "D"), sum(k for k, c in ops if c != "I")


def concat(*parts):
    """Join lists of runs; equal neighbouring ops at a seam become one run (reference: concat in edlib_adj_align)."""
    out = []
    for part in parts:
        for k, c in part:
            if out and out[-1][1] == c:
                out[-1] = (out[-1][0] + k, c)
            elif k:
                out.append((k, c))
    return out


def first_long_match(ops):
    return next((x for x, (k, c) in enumerate(ops) if c == "=" and k >= NUM_MATCH), None)


def trim(ops):
    """Drop runs from both ends until an '=' run of NUM_MATCH or more -> (runs, query bases cut at the start, reference bases cut at
    the start, query bases cut at the end, reference bases cut at the end); no such run: no runs (reference: trim_while, twice)."""
    first = first_long_match(ops)
    if first is None:
        return [], *lengths(ops), 0, 0
    last = len(ops) - 1 - first_long_match(ops[::-1])
    return ops[first:last + 1], *lengths(ops[:first]), *lengths(ops[last + 1:])


def consensus(ops, temp_seq, temp_q, comp_seq, comp_q):
    """Column by column over the alignment of the template (query) and the reverse-complemented complement (reference): the base
    with the higher adjusted score wins, the template on a tie; agreeing columns get the sum; a gap column takes the score of the
    last base consumed on the gap's side; a chosen gap is dropped (reference: compute_consensus) -> (sequence, quality string)."""
    col = np.repeat(["=XID".index(c) for _, c in ops], [k for k, _ in ops])
    on_t, on_c = col != 3, col != 2
    t = np.full(len(col), GAP, np.uint8)
    c = np.full(len(col), GAP, np.uint8)
    t[on_t] = np.frombuffer(temp_seq.encode("ascii"), np.uint8)
    c[on_c] = np.frombuffer(comp_seq.encode("ascii"), np.uint8)
    tq = np.asarray(temp_q, np.float32)[np.maximum(np.cumsum(on_t) - 1, 0)]
    cq = np.asarray(comp_q, np.float32)[np.maximum(np.cumsum(on_c) - 1, 0)]
    take_c = cq > tq
    base = np.where(take_c, c, t)
    q = np.where(t == c, tq + cq, np.where(take_c, cq, tq))
    keep = base != GAP
    quals = np.round(np.clip(q[keep], 0, 60) + 33).astype(np.uint8)
    return base[keep].tobytes().decode("ascii"), quals.tobytes().decode("ascii")


class DeviceAligners:
    """The two batched alignments of the pipeline -> per pair a CIGAR string or its runs as [(length, op)]. ``nw`` gives None for a
    pair that was not aligned."""

    def __init__(self, device="cuda"):
        self.device = device

    def nw(self, queries, refs):
        got = al.nw_align(queries, refs, cigar=True, device=self.device)
        return [got.ops(i) if got.status[i] == al.NW_OK else None for i in range(len(got))]

    def sg(self, queries, refs):
        return al.sg_align(queries, refs, cigar=True, device=self.device).cigar


def _fits(q, r):
    return max(len(q), len(r)) <= al.MAX_LEN


def adj_align(queries, refs, device="cuda", stats=None, aligners=None):
    """The global alignment of every pair with both ends repaired by the semi-global one -> a list of run lists, None where a pair
    has no '=' run of NUM_MATCH, is longer than the semi-global limit and so cannot be aligned whole (reference: edlib_adj_align).
    ``stats`` (a dict) counts 'kept_nw' (an end or a whole pair over the limit that keeps its global CIGAR) and 'unaligned'.
    ``aligners``: an object with the two methods of ``DeviceAligners`` (the tests of the host code pass a restatement)."""
    aligners = aligners or DeviceAligners(device)
    stats = stats if stats is not None else {}
    stats.setdefault("kept_nw", 0)
    stats.setdefault("unaligned", 0)
    n = len(queries)
    ops = [c if c is None or isinstance(c, list) else parse_cigar(c) for c in aligners.nw(queries, refs)] if n else []
    stats["unaligned"] += sum(o is None for o in ops)
    done = [o is None for o in ops]
    for end in ("head", "tail"):
        jobs, where = [], []
        for i in range(n):
            if done[i]:
                continue
            q, r = queries[i], refs[i]
            o = ops[i] if end == "head" else ops[i][::-1]
            x = first_long_match(o)
            if x is None:                                    # nothing to anchor on: the whole pair
                done[i] = True
                if _fits(q, r):
                    jobs.append((q, r)); where.append((i, None))
                else:
                    ops[i] = None
                    stats["unaligned"] += 1
            elif x > 0:
                ql, rl = lengths(o[:x + 1])
                part = (q[:ql], r[:rl]) if end == "head" else (q[len(q) - ql:], r[len(r) - rl:])
                if _fits(*part):
                    jobs.append(part); where.append((i, x))
                else:
                    stats["kept_nw"] += 1
        cigars = aligners.sg([q for q, _ in jobs], [r for _, r in jobs]) if jobs else []
        for (i, x), runs in zip(where, map(parse_cigar, cigars)):
            if x is None:
                ops[i] = runs
            elif end == "head":
                ops[i] = concat(runs, ops[i][x + 1:])
            else:
                ops[i] = concat(ops[i][:len(ops[i]) - (x + 1)], runs)
    return ops


def call_pairs(temp_seqs, temp_qstrings, comp_seqs, comp_qstrings, device="cuda", stats=None, aligners=None):
    """Duplex consensus of (template, complement) calls: sequences over ACGT with their FASTQ quality strings (Phred + 33) -> a list of
    (sequence, quality string), ("", "") where nothing survives the trim (reference: call_basespace_duplex per pair)."""
    n = len(temp_seqs)
    if not (len(temp_qstrings) == len(comp_seqs) == len(comp_qstrings) == n):
        raise ValueError("call_pairs: the four lists must have one entry per pair")

    def phred(qstring, seq):
        q = np.frombuffer(qstring.encode("latin-1"), np.uint8)
        if len(q) != len(seq):
            raise ValueError("call_pairs: a quality string of %d for %d bases" % (len(q), len(seq)))
        return q - np.uint8(33)

    temp_q = [adjust_qscores(phred(q, s), s, 1) for q, s in zip(temp_qstrings, temp_seqs)]
    comp_q = [adjust_qscores(phred(q, s), s, -1)[::-1] for q, s in zip(comp_qstrings, comp_seqs)]
    comp_rc = [revcomp(s) for s in comp_seqs]
    stats = stats if stats is not None else {}
    long = [i for i in range(n) if max(len(temp_seqs[i]), len(comp_rc[i])) > al.NW_MAX_LEN]
    stats["unaligned"] = stats.get("unaligned", 0) + len(long)
    todo = sorted(set(range(n)) - set(long))
    aligned = adj_align([temp_seqs[i] for i in todo], [comp_rc[i] for i in todo], device=device, stats=stats,
                        aligners=aligners)
    out = [("", "")] * n
    for i, ops in zip(todo, aligned):
        if ops is None:
            continue
        ops, ts, cs, te, ce = trim(ops)
        if not ops:
            continue
        t, c = temp_seqs[i], comp_rc[i]
        out[i] = consensus(ops, t[ts:len(t) - te], temp_q[i][ts:len(t) - te], c[cs:len(c) - ce], comp_q[i][cs:len(c) - ce])
    return out


def report(stats, fd=sys.stderr):
    if stats.get("kept_nw"):
        fd.write("> read ends over %d bases kept without end repair: %d\n" % (al.MAX_LEN, stats["kept_nw"]))
    if stats.get("unaligned"):
        fd.write("> pairs without a long match over the alignment limits (empty call): %d\n" % stats["unaligned"])

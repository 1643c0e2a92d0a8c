"""Plain restatements of what the duplex caller is made of ("Duplex"), used by tests/test_duplex_cpu.py,
tests/test_gpu_duplex.py and tests/golden/make_golden_duplex.py: the global alignment under unit costs, the semi-global affine
alignment (both with full matrices, filled over anti-diagonals as tests/align_ref.py does, the traceback comparing matrix VALUES), an
edit distance on three rolling anti-diagonals for pairs too long for a matrix, and the pair pipeline in plain Python.

Global (``nw``), query q of m bases against reference r of n, 1-based:
    D(0,0) = 0, D(i,0) = i, D(0,j) = j
    D(i,j) = min(D(i-1,j-1) + [q_i != r_j], D(i,j-1) + 1 (D: consumes a ref base), D(i-1,j) + 1 (I: consumes a query base))
    Traceback from (m,n) to (0,0): among the predecessors that attain the minimum the diagonal first, then D, then I.

Semi-global (``sg``): the recurrences of align_ref without the floor at 0, H(i,0) = H(0,j) = 0, E and F start at -infinity. End cell:
the largest H over the last row and the last column, among equals the smallest i, then the smallest j. Traceback: the diagonal, then E,
then F; in E / F the open wins a tie; stop on reaching row 0 or column 0. The CIGAR covers both sequences completely: the unaligned
head and tail come out as one I or D run each.
"""
import re

import numpy as np

from align_ref import compress, parse, _codes

NEG = -(1 << 40)
SG_DEFAULT = (5, -4, 10, 2)                        # match, mismatch, gap_open, gap_extend
NUM_MATCH = 11                                    # an '=' run of this length anchors the end repair and the trim


def nw_fill(seq, ref):
    """-> D as int64 [m + 1, n + 1]"""
    a, b = _codes(seq), _codes(ref)
    m, n = len(a), len(b)
    D = np.zeros((m + 1, n + 1), np.int64)
    D[:, 0] = np.arange(m + 1)
    D[0, :] = np.arange(n + 1)
    for d in range(2, m + n + 1):
        i = np.arange(max(1, d - n), min(m, d - 1) + 1)
        j = d - i
        D[i, j] = np.minimum(D[i - 1, j - 1] + (a[i - 1] != b[j - 1]), np.minimum(D[i, j - 1], D[i - 1, j]) + 1)
    return D


def nw(seq, ref):
    """-> ([distance, =, X, I, D, runs], CIGAR)"""
    D = nw_fill(seq, ref)
    i, j = len(seq), len(ref)
    ops = []
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i, j] == D[i - 1, j - 1] + (seq[i - 1] != ref[j - 1]):
            ops.append("=" if seq[i - 1] == ref[j - 1] else "X")
            i, j = i - 1, j - 1
        elif j > 0 and D[i, j] == D[i, j - 1] + 1:
            ops.append("D")
            j -= 1
        else:
            assert i > 0 and D[i, j] == D[i - 1, j] + 1
            ops.append("I")
            i -= 1
    ops.reverse()
    cigar = compress(ops)
    return [int(D[len(seq), len(ref)])] + [ops.count(c) for c in "=XID"] + [len(parse(cigar))], cigar


def edit_distance(seq, ref):
    """D(m, n) of the same recurrence on three rolling anti-diagonals (no matrix): for pairs of tens of thousands of bases."""
    a, b = _codes(seq), _codes(ref)
    m, n = len(a), len(b)
    if m == 0 or n == 0:
        return m + n
    big = m + n + 1
    prev2 = np.full(m + 1, big, np.int64)             # anti-diagonal d - 2, indexed by i
    prev = np.full(m + 1, big, np.int64)              # anti-diagonal d - 1
    prev2[0] = 0                                      # d = 0: D(0,0)
    prev[0] = 1                                       # d = 1: D(0,1), D(1,0)
    prev[1] = 1
    for d in range(2, m + n + 1):
        cur = np.full(m + 1, big, np.int64)
        if d <= n:
            cur[0] = d
        if d <= m:
            cur[d] = d
        i = np.arange(max(1, d - n), min(m, d - 1) + 1)
        j = d - i
        cur[i] = np.minimum(prev2[i - 1] + (a[i - 1] != b[j - 1]), np.minimum(prev[i], prev[i - 1]) + 1)
        prev2, prev = prev, cur
    return int(prev[m])


def sg_fill(seq, ref, match=5, mismatch=-4, gap_open=10, gap_extend=2):
    a, b = _codes(seq), _codes(ref)
    m, n = len(a), len(b)
    H = np.zeros((m + 1, n + 1), np.int64)
    E = np.full((m + 1, n + 1), NEG, np.int64)
    F = np.full((m + 1, n + 1), NEG, np.int64)
    for d in range(2, m + n + 1):
        i = np.arange(max(1, d - n), min(m, d - 1) + 1)
        j = d - i
        s = np.where(a[i - 1] == b[j - 1], match, mismatch)
        e = np.maximum(H[i, j - 1] - gap_open, E[i, j - 1] - gap_extend)
        f = np.maximum(H[i - 1, j] - gap_open, F[i - 1, j] - gap_extend)
        E[i, j], F[i, j] = e, f
        H[i, j] = np.maximum(H[i - 1, j - 1] + s, np.maximum(e, f))
    return H, E, F


def sg(seq, ref, match=5, mismatch=-4, gap_open=10, gap_extend=2):
    """-> (the ten integers of align_ref.COLUMNS, CIGAR over both sequences). The counts include the overhang runs; the start / end
    columns describe the aligned part."""
    m, n = len(seq), len(ref)
    if m == 0 or n == 0:
        cigar = "%dI" % m if m else "%dD" % n if n else ""
        return [0, 0, 0, m, n, 0, -1, 0, -1, int(m + n > 0)], cigar
    H, E, F = sg_fill(seq, ref, match, mismatch, gap_open, gap_extend)
    cells = [(i, n) for i in range(1, m + 1)] + [(m, j) for j in range(1, n + 1)]
    score = max(int(H[c]) for c in cells)
    i, j = min(c for c in cells if H[c] == score)       # the smallest i, then the smallest j
    end_i, end_j = i, j
    ops, state = ["D"] * (n - j) + ["I"] * (m - i), "H"
    while i > 0 and j > 0:
        if state == "H":
            s = match if seq[i - 1] == ref[j - 1] else mismatch
            if H[i, j] == H[i - 1, j - 1] + s:
                ops.append("=" if seq[i - 1] == ref[j - 1] else "X")
                i, j = i - 1, j - 1
            elif H[i, j] == E[i, j]:
                state = "E"
            else:
                assert H[i, j] == F[i, j]
                state = "F"
        elif state == "E":
            ops.append("D")
            state = "H" if E[i, j] == H[i, j - 1] - gap_open else "E"
            j -= 1
        else:
            ops.append("I")
            state = "H" if F[i, j] == H[i - 1, j] - gap_open else "F"
            i -= 1
    ops += ["I"] * i + ["D"] * j
    ops.reverse()
    cigar = compress(ops)
    return [score] + [ops.count(c) for c in "=XID"] + [j, end_j - 1, i, end_i - 1, len(parse(cigar))], cigar


# ---- the pair pipeline, in plain Python ------------------------------------------------------------------------------------------

def revcomp(seq):
    return seq[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def adj_qscores(q, seq, qshift, pool=5):
    """Phred scores (integers) -> float32: shifted by `qshift` positions with the edge value repeated (+1 towards the end, -1 towards
    the start), an edge-padded minimum over `pool` positions, then the mean over every homopolymer run of two or more bases."""
    q = [int(v) for v in q]
    n = len(q)
    shifted = [q[min(max(i - qshift, 0), n - 1)] for i in range(n)]
    half = pool // 2
    out = np.array([min(shifted[min(max(i + o, 0), n - 1)] for o in range(-half, half + 1)) for i in range(n)], np.float32)
    for run in re.finditer(r"(.)\1+", seq):
        st, en = run.span()
        out[st:en] = np.mean(out[st:en])
    return out


def lengths(ops):
    """[(length, op)] -> (query bases, reference bases) consumed"""
    return sum(k for k, c in ops if c in "=XI"), sum(k for k, c in ops if c in "=XD")


def concat(*parts):
    """Join lists of runs, merging equal neighbouring ops at the seams."""
    out = []
    for part in parts:
        for k, c in part:
            if out and out[-1][1] == c:
                out[-1] = (out[-1][0] + k, c)
            else:
                out.append((k, c))
    return out


def _first_long(ops):
    return next((x for x, (k, c) in enumerate(ops) if c == "=" and k >= NUM_MATCH), None)


def adj_align(query, ref, nw_cigar=None, sg_cigar=None):
    """The global alignment with both ends repaired by the semi-global one -> [(length, op)]. The head is everything up to and
    including the first '=' run of 11 or more, the tail everything from the last such run on; a pair without such a run is aligned
    whole by the semi-global aligner."""
    nw_cigar = nw_cigar or (lambda q, r: nw(q, r)[1])
    sg_cigar = sg_cigar or (lambda q, r: sg(q, r)[1])
    ops = parse(nw_cigar(query, ref))
    first = _first_long(ops)
    if first is None:
        return parse(sg_cigar(query, ref))
    if first > 0:
        qs, rs = lengths(ops[:first + 1])
        ops = concat(parse(sg_cigar(query[:qs], ref[:rs])), ops[first + 1:])
    last = _first_long(ops[::-1])
    if last is None:
        return parse(sg_cigar(query, ref))
    if last > 0:
        qe, re_ = lengths(ops[-(last + 1):])
        ops = concat(ops[:-(last + 1)], parse(sg_cigar(query[len(query) - qe:], ref[len(ref) - re_:])))
    return ops


def trim(ops):
    """Drop runs from both ends until an '=' run of 11 or more -> (runs, query bases cut at the start, reference bases cut at the
    start, query bases cut at the end, reference bases cut at the end)."""
    first = _first_long(ops)
    if first is None:
        return [], *lengths(ops), 0, 0
    qs, rs = lengths(ops[:first])
    ops = ops[first:]
    last = _first_long(ops[::-1])
    qe, re_ = lengths(ops[len(ops) - last:])
    return ops[:len(ops) - last], qs, rs, qe, re_


def consensus(ops, temp_seq, temp_q, comp_seq, comp_q):
    """Column by column: the base with the higher adjusted score (the template on a tie); agreeing columns get the sum; a gap column
    compares against the score of the last base consumed on the gap's side (the first base if none was), and a chosen gap is dropped."""
    out, quals = [], []
    ti = ci = 0
    for k, c in ops:
        for _ in range(k):
            tb = temp_seq[ti] if c in "=XI" else "-"
            cb = comp_seq[ci] if c in "=XD" else "-"
            ti += c in "=XI"
            ci += c in "=XD"
            tq, cq = np.float32(temp_q[max(ti - 1, 0)]), np.float32(comp_q[max(ci - 1, 0)])
            base, q = (cb, cq) if cq > tq else (tb, tq)
            if tb == cb:
                q = np.float32(tq + cq)
            if base != "-":
                out.append(base)
                quals.append(q)
    q = np.round(np.clip(np.array(quals, np.float32), 0, 60) + 33).astype(np.uint8)
    return "".join(out), q.tobytes().decode("ascii")


def call_pair(temp_seq, temp_q, comp_seq, comp_q, nw_cigar=None, sg_cigar=None):
    """One (template, complement) pair of calls with their Phred scores (integers) -> (consensus sequence, quality string)."""
    tq = adj_qscores(temp_q, temp_seq, 1)
    cq = adj_qscores(comp_q, comp_seq, -1)[::-1]
    comp_seq = revcomp(comp_seq)
    ops, ts, cs, te, ce = trim(adj_align(temp_seq, comp_seq, nw_cigar, sg_cigar))
    if not ops:
        return "", ""
    return consensus(ops, temp_seq[ts:len(temp_seq) - te], tq[ts:len(tq) - te], comp_seq[cs:len(comp_seq) - ce],
                     cq[cs:len(cq) - ce])

"""The read mapper, restated in plain Python / numpy with integer arithmetic only ("Mapper"). This file DEFINES
what ``bonito_amd.aligner`` and csrc/mapper.hip compute; tests/test_mapper_cpu.py and tests/test_gpu_mapper.py compare against it
bit for bit. Parity with minimap2 is not claimed anywhere: seeds, chain scores, mapq, end extension and tie-breaks are this file's.

Sketch: (k, w)-minimizers, 11 <= k <= 28, 1 <= w <= 64. A base is A, C, G, T = 0, 1, 2, 3; the k-mer ending at position p has the
    forward value sum(base[p - k + 1 + t] << 2 (k - 1 - t)) and the reverse-complement value sum((3 - base[p - k + 1 + t]) << 2 t).
    key(x) = MIX(x) (below: an invertible map of the 2k-bit integers), the k-mer's key is the smaller of the two keys and its strand
    bit says that the reverse-complement key was the smaller one. A k-mer with a base outside ACGT, or whose two keys are equal (its
    two values are then equal: the mix is invertible), has no key. The window that ENDS at k-mer position p holds the k-mer positions
    max(k - 1, p - w + 1) .. p; windows end at every p >= min(k + w - 2, L - 1) (a sequence with fewer than w k-mers has the one window
    that holds them all). A window selects the leftmost position among those with its smallest key, nothing if none has a key. The
    minimizers of a sequence are the distinct selected positions in increasing order: (key, position of the k-mer's LAST base, strand).
Index: the minimizers of every contig, sorted by (key, contig, position). A key with more than max_occ occurrences seeds nothing.
Seeds: a query minimizer (key, qpos, qs) gives one anchor per occurrence (contig, rpos, rs): strand = qs xor rs, and
    qpos' = qpos on strand 0, len(query) - qpos + k - 2 on strand 1 (the last base of the same k-mer on the reverse-complemented
    query). The anchors of a read are sorted by (strand, contig, rpos, qpos').
Chain: f[i] = max(k, max_j f[j] + min(dq, dr, k) - cost(|dr - dq|)) over the at most 64 anchors j = i - 64 .. i - 1 with the same
    strand and contig, 0 < dq <= max_dist, 0 < dr <= max_dist, |dr - dq| <= bandwidth; cost(0) = 0,
    cost(g) = ((5 g) >> 5) + (floor(log2 g) >> 1). A predecessor is taken only when its score is GREATER than k; among equal scores
    the largest j. The primary chain ends at the anchor with the largest f (the smallest index among equals). s2 is the largest f
    among the anchors on another strand or contig or whose rpos lies outside [rpos of the chain's first anchor, rpos of its last], 0
    if there is none. Accepted with at least min_cnt anchors and s1 >= min_score; mapq = min(60, 60 (s1 - s2) // s1), halved
    (rounding down) when the chain has fewer than 10 anchors.
Base alignment: on the aligned strand (the query reverse-complemented on strand 1) the span starts at the first base of the first
    anchor's k-mer and ends behind the last anchor's last base, in query and reference alike; it is widened at either end while the
    neighbouring query and reference bases are equal bases of ACGT, up to the read's or contig's end. Cuts: while more than 16384
    query bases remain from the start of the piece to the end of the span, the piece ends behind the last base of the last chain
    anchor that keeps it at 16384 query bases or fewer (no cut where no such anchor is left). Every piece is aligned globally under unit costs (tests/duplex_ref.py ``nw``:
    diagonal, then D, then I), bases outside ACGT standing in as A; the CIGARs are joined, = and X become M, equal neighbours merge.
    NM, MD, mlen (matching columns) and blen (all columns) are taken against the true sequences: a column with a base outside ACGT
    is a mismatch.
Record: mappy's field names. r_st / r_en and the CIGAR are on the reference strand; q_st / q_en are positions on the read AS GIVEN
    (on strand -1: length - end and length - start of the aligned-strand span), which is what mappy reports and what the reference's
    sam_record and summary_row assume when they swap the soft-clips and subtract from the length on the minus strand.
"""
import numpy as np

H = 64
PIECE = 16384
DEFAULTS = dict(k=15, w=10, max_occ=64, max_dist=5000, bandwidth=500, min_cnt=3, min_score=40)
_LUT = np.full(256, 4, np.uint8)
_LUT[np.frombuffer(b"ACGT", np.uint8)] = (0, 1, 2, 3)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_M64 = (1 << 64) - 1


def mix(x, mask):
    """The key of a 2k-bit value (Python integers): seven invertible steps modulo 2^(2k) - adding shifted copies of itself (an odd
    multiplier), xor with a right shift of itself, and one complement."""
    x = (~x + (x << 21)) & mask
    x = x ^ (x >> 24)
    x = (x + (x << 3) + (x << 8)) & mask
    x = x ^ (x >> 14)
    x = (x + (x << 2) + (x << 4)) & mask
    x = x ^ (x >> 28)
    x = (x + (x << 31)) & mask
    return x


def _mix_np(x, mask):
    u = np.uint64
    m = u(mask)
    x = (~x + (x << u(21))) & m
    x = x ^ (x >> u(24))
    x = (x + (x << u(3)) + (x << u(8))) & m
    x = x ^ (x >> u(14))
    x = (x + (x << u(2)) + (x << u(4))) & m
    x = x ^ (x >> u(28))
    x = (x + (x << u(31))) & m
    return x


def codes(seq):
    return _LUT[np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), np.uint8)]


def revcomp(seq):
    return seq.encode().translate(_COMP)[::-1].decode()


def check_kw(k, w):
    if not 11 <= k <= 28:
        raise ValueError("k must be in 11..28")
    if not 1 <= w <= 64:
        raise ValueError("w must be in 1..64")


def sketch(seq, k=15, w=10):
    """-> [(key, position of the k-mer's last base, strand bit)] in position order"""
    check_kw(k, w)
    c = codes(seq)
    n = len(c) - k + 1                                # k-mer positions, index u = p - (k - 1)
    if n < 1:
        return []
    u64 = np.uint64
    mask = (1 << (2 * k)) - 1
    fw, rv, bad = np.zeros(n, u64), np.zeros(n, u64), np.zeros(n, bool)
    with np.errstate(over="ignore"):
        for t in range(k):
            b = c[t:t + n]
            bad |= b > 3
            b = (b & 3).astype(u64)
            fw |= b << u64(2 * (k - 1 - t))
            rv |= (u64(3) - b) << u64(2 * t)
        kf, kr = _mix_np(fw, mask), _mix_np(rv, mask)
    none = u64(_M64)
    key = np.where(bad | (kf == kr), none, np.minimum(kf, kr))
    strand = kr < kf
    ww = min(w, n)
    start = np.arange(n - ww + 1)
    best, arg = key[start], start.copy()
    for o in range(1, ww):
        cand = key[start + o]
        better = cand < best                          # strictly: the leftmost of equal keys stays
        best, arg = np.where(better, cand, best), np.where(better, start + o, arg)
    sel = np.unique(arg[best != none])
    return [(int(key[x]), int(x) + k - 1, int(strand[x])) for x in sel]


class Index:
    """contigs: [(name, sequence)] -> the sorted minimizer table and, per key that seeds, its occurrences (contig, pos, strand)."""

    def __init__(self, contigs, k=15, w=10, max_occ=64):
        self.k, self.w, self.max_occ = k, w, max_occ
        self.names = [n for n, _ in contigs]
        self.seqs = [s for _, s in contigs]
        if sum(len(s) for s in self.seqs) >= 1 << 31:
            raise ValueError("the reference must be shorter than 2^31 bases")
        table = []
        for ci, s in enumerate(self.seqs):
            table.extend((key, ci, pos, st) for key, pos, st in sketch(s, k, w))
        table.sort()
        self.table = table
        self.occ = {}
        for key, ci, pos, st in table:
            self.occ.setdefault(key, []).append((ci, pos, st))
        self.seeding = {key: v for key, v in self.occ.items() if len(v) <= max_occ}


def seed(minimizers, qlen, index):
    """minimizers of one query -> its anchors (strand, contig, rpos, qpos'), sorted"""
    out = []
    for key, qpos, qs in minimizers:
        for ci, rpos, rs in index.seeding.get(key, ()):
            st = qs ^ rs
            out.append((st, ci, rpos, qpos if st == 0 else qlen - qpos + index.k - 2))
    out.sort()
    return out


def cost(g):
    return 0 if g == 0 else ((5 * g) >> 5) + ((g.bit_length() - 1) >> 1)


def chain_dp(anchors, k=15, max_dist=5000, bandwidth=500):
    """-> (f, p): the score of the best chain ending at every anchor and its predecessor (-1: none)"""
    f, p = [], []
    for i, (st, ci, r, q) in enumerate(anchors):
        best, arg = k, -1
        for j in range(max(0, i - H), i):
            sj, cj, rj, qj = anchors[j]
            dr, dq = r - rj, q - qj
            if sj != st or cj != ci or not 0 < dq <= max_dist or not 0 < dr <= max_dist or abs(dr - dq) > bandwidth:
                continue
            sc = f[j] + min(dq, dr, k) - cost(abs(dr - dq))
            if sc > k and sc >= best and (sc > best or arg < j):
                best, arg = sc, j
        f.append(best)
        p.append(arg)
    return f, p


def chain(anchors, k=15, max_dist=5000, bandwidth=500):
    """-> (indices of the primary chain's anchors in increasing order, s1, s2); ([], 0, 0) without anchors"""
    if not anchors:
        return [], 0, 0
    f, p = chain_dp(anchors, k, max_dist, bandwidth)
    s1 = max(f)
    i = f.index(s1)
    idx = []
    while i >= 0:
        idx.append(i)
        i = p[i]
    idx.reverse()
    st, ci, lo, hi = anchors[idx[0]][0], anchors[idx[0]][1], anchors[idx[0]][2], anchors[idx[-1]][2]
    s2 = max([f[j] for j, (sj, cj, rj, _) in enumerate(anchors) if sj != st or cj != ci or rj < lo or rj > hi] + [0])
    return idx, s1, s2


def mapq_of(s1, s2, cnt):
    mq = min(60, (60 * (s1 - s2)) // s1)
    return mq // 2 if cnt < 10 else mq


# ---- banded global alignment with the values kept: tests/duplex_ref.py ``nw`` for pieces too long for a full matrix ---------------

_INF = 1 << 29


def nw_ops(seq, ref):
    """Global alignment under unit costs of two code arrays (equal codes match) -> [(length, op)] over '=XID', the recurrence, band
    rule and tie-breaks of duplex_ref.nw / csrc/nw.hip: the band's half-width doubles from 64 until floor((d - |delta|) / 2) <= k,
    at which distance and traceback equal those of the full matrix."""
    a, b = np.asarray(seq, np.int64), np.asarray(ref, np.int64)
    m, n = len(a), len(b)
    if m == 0 or n == 0:
        return [(m, "I")] if m else [(n, "D")] if n else []
    delta = n - m
    k = 64
    while True:
        lo, hi = min(0, delta) - k, max(0, delta) + k
        W = hi - lo + 1
        D = np.full((m + 1, W + 1), _INF, np.int32)    # D[i, c]: the cell (i, j = i + lo + c); column W stays infinite
        off = np.arange(W)
        j0 = lo + off                                 # j of row 0
        D[0, :W] = np.where((j0 >= 0) & (j0 <= n), j0, _INF)
        bpad = np.concatenate([np.full(W + 1, -1), b, np.full(W + 1, -1)])
        for i in range(1, m + 1):
            j = i + lo + off
            inside = (j >= 1) & (j <= n)
            rb = bpad[W + 1 + i + lo - 1: W + 1 + i + lo - 1 + W]      # b[j - 1]
            t = np.minimum(D[i - 1, :W] + (rb != a[i - 1]), D[i - 1, 1:] + 1)
            t = np.where(inside, t, _INF)
            if lo + i <= 0 <= hi + i:                 # the border D(i, 0) = i inside the band
                t[-(i + lo)] = i
            row = np.minimum.accumulate(t - off) + off
            D[i, :W] = np.where(inside | (j == 0), np.minimum(row, _INF), _INF)
        d = int(D[m, n - m - lo])
        if (d - abs(delta)) // 2 <= k:
            break
        k *= 2
    ops = []
    i, j = m, n
    while i > 0 or j > 0:
        c = j - i - lo
        if i > 0 and j > 0 and D[i, c] == D[i - 1, c] + (a[i - 1] != b[j - 1]):
            ops.append("=" if a[i - 1] == b[j - 1] else "X")
            i, j = i - 1, j - 1
        elif j > 0 and c > 0 and D[i, c] == D[i, c - 1] + 1:
            ops.append("D")
            j -= 1
        else:
            assert i > 0 and D[i, c] == D[i - 1, c + 1] + 1
            ops.append("I")
            i -= 1
    ops.reverse()
    runs = []
    for o in ops:
        if runs and runs[-1][1] == o:
            runs[-1][0] += 1
        else:
            runs.append([1, o])
    return [(n_, o) for n_, o in runs]


# ---- one read -----------------------------------------------------------------------------------------------------------------

def span_and_pieces(chain_anchors, k, q, r):
    """chain anchors [(rpos, qpos')] on the aligned strand, code arrays q and r (the contig) -> (q_st, q_en, r_st, r_en, pieces as
    (q0, q1, r0, r1))"""
    r_st, q_st = chain_anchors[0][0] - k + 1, chain_anchors[0][1] - k + 1
    r_en, q_en = chain_anchors[-1][0] + 1, chain_anchors[-1][1] + 1
    while q_st > 0 and r_st > 0 and q[q_st - 1] == r[r_st - 1] and q[q_st - 1] < 4:
        q_st, r_st = q_st - 1, r_st - 1
    while q_en < len(q) and r_en < len(r) and q[q_en] == r[r_en] and q[q_en] < 4:
        q_en, r_en = q_en + 1, r_en + 1
    pieces, q0, r0, x = [], q_st, r_st, 0
    while q_en - q0 > PIECE:
        cut = None
        while x < len(chain_anchors) and chain_anchors[x][1] + 1 - q0 <= PIECE:
            if chain_anchors[x][1] + 1 > q0:
                cut = chain_anchors[x]
            x += 1
        if cut is None:                               # no anchor left to cut at: the last piece is longer
            break
        pieces.append((q0, cut[1] + 1, r0, cut[0] + 1))
        q0, r0 = cut[1] + 1, cut[0] + 1
    pieces.append((q0, q_en, r0, r_en))
    return q_st, q_en, r_st, r_en, pieces


def finish(cigar, q, r, q_st, r_st):
    """[(count, op)] over M I D (0 1 2), code arrays -> (NM, MD, mlen, blen) against the true bases"""
    letters = "ACGTN"
    nm = mlen = blen = run = 0
    md = []
    qi, ri = q_st, r_st
    for cnt, op in cigar:
        blen += cnt
        if op == 0:
            for _ in range(cnt):
                if q[qi] == r[ri] and q[qi] < 4:
                    run += 1
                    mlen += 1
                else:
                    md.append("%d%s" % (run, letters[r[ri]]))
                    run = 0
                    nm += 1
                qi, ri = qi + 1, ri + 1
        elif op == 1:
            nm += cnt
            qi += cnt
        else:
            md.append("%d^%s" % (run, "".join(letters[x] for x in r[ri:ri + cnt])))
            run = 0
            nm += cnt
            ri += cnt
    md.append("%d" % run)
    return nm, "".join(md), mlen, blen


def map_anchors(anchors, seq, index, max_dist=5000, bandwidth=500, min_cnt=3, min_score=40):
    """The sorted anchors of one read -> its record (a dict with mappy's field names) or None"""
    k = index.k
    idx, s1, s2 = chain(anchors, k, max_dist, bandwidth)
    if len(idx) < min_cnt or s1 < min_score:
        return None
    st, ci = anchors[idx[0]][:2]
    ca = [(anchors[i][2], anchors[i][3]) for i in idx]
    q = codes(revcomp(seq) if st else seq)
    r = codes(index.seqs[ci])
    q_st, q_en, r_st, r_en, pieces = span_and_pieces(ca, k, q, r)
    qa, ra = np.where(q > 3, 0, q), np.where(r > 3, 0, r)
    cigar = []
    for q0, q1, r0, r1 in pieces:
        for cnt, o in nw_ops(qa[q0:q1], ra[r0:r1]):
            op = {"=": 0, "X": 0, "I": 1, "D": 2}[o]
            if cigar and cigar[-1][1] == op:
                cigar[-1] = (cigar[-1][0] + cnt, op)
            else:
                cigar.append((cnt, op))
    nm, md, mlen, blen = finish(cigar, q, r, q_st, r_st)
    if st:                                            # reported on the read as given, like mappy's (the CIGAR stays on the aligned strand)
        q_st, q_en = len(q) - q_en, len(q) - q_st
    return dict(ctg=index.names[ci], r_st=r_st, r_en=r_en, q_st=q_st, q_en=q_en, strand=-1 if st else 1,
                mapq=mapq_of(s1, s2, len(idx)), cigar=[(c, o) for c, o in cigar],
                cigar_str="".join("%d%s" % (c, "MID"[o]) for c, o in cigar), NM=nm, MD=md, mlen=mlen, blen=blen)


def map_read(seq, index, **chain_kw):
    seq = seq.upper()
    return map_anchors(seed(sketch(seq, index.k, index.w), len(seq), index), seq, index, **chain_kw)

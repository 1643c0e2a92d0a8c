"""End extension of the read mapper, restated in plain Python with integer arithmetic only ("Mapper"). This file
DEFINES what ``bh_map_extend`` (csrc/mapper.hip) and ``Aligner.map_batch(extend_ends=True)`` compute on top of tests/mapper_ref.py,
which it imports and does not change; tests/test_mapper_ext_cpu.py and tests/test_gpu_mapper_ext.py compare against it bit for bit.

Tails: for one end of one mapping, on the aligned strand, after ``span_and_pieces`` has widened the span:
    right end: Q = q[q_en : min(len(q), q_en + EXT_MAX)], R = r[r_en : min(len(r), r_en + len(Q) + EXT_BAND)] with r the CONTIG;
    left end: the same on the reversed tails, Q = reversed(q[max(0, q_st - EXT_MAX) : q_st]),
    R = reversed(r[max(0, r_st - len(Q) - EXT_BAND) : r_st]).
Recurrence: S(0,0) = 0; only the cells with |j - i| <= EXT_BAND exist, every other cell is minus infinity;
    S(i,j) = max(S(i-1,j-1) + (+2 if Q[i-1] == R[j-1] and it is one of ACGT else -4), S(i-1,j) - 4, S(i,j-1) - 4).
    The borders follow from the same rule (S(i,0) = -4 i, S(0,j) = -4 j inside the band). A base outside ACGT never matches.
End cell: the cell with the largest S, (0,0) included; among equals the smallest i + j, then the smallest i. (0,0): no extension.
Path: from the end cell back to (0,0); where several predecessors explain a cell's value the diagonal, then (i-1,j) (a query base
    alone, I), then (i,j-1) (D). It is emitted as run words count << 2 | op over = X I D = 0 1 2 3, what ``aligner.finish`` takes;
    for the left end in read order, so that left runs + span runs + right runs is the whole alignment.
Record: q_st, q_en, r_st, r_en move outwards by the extended lengths; cigar, cigar_str, NM, MD, mlen, blen come from one ``finish``
    over the joined runs; the strand flip of q_st / q_en, mapq and the chain stay as they are.
"""
import mapper_ref as M

EXT_MAX = 512
EXT_BAND = 32
MATCH, PENALTY = 2, 4
_NONE = -(1 << 40)


def extend(Q, R):
    """Code sequences (0..3 = A C G T, anything else no base) of the two tails, nearest base first -> (score, i, j, ops): the end
    cell and the path's ops from the END CELL BACK to (0,0) as a string over '=XID'. Cells outside the band do not exist."""
    m, n, B = len(Q), len(R), EXT_BAND
    S = [[_NONE] * (2 * B + 1) for _ in range(m + 1)]              # S[i][j - i + B]
    T = [[0] * (2 * B + 1) for _ in range(m + 1)]                  # 0 diagonal, 1 from (i-1, j), 2 from (i, j-1)
    S[0][B] = 0
    best = (0, 0, 0, 0)                                            # (S, -(i + j), -i) is maximised; kept as (S, i + j, i, j)
    for i in range(m + 1):
        row, trow = S[i], T[i]
        up = S[i - 1] if i else None
        for c in range(2 * B + 1):
            j = i + c - B
            if j < 0 or j > n or (i == 0 and j == 0):
                continue
            v, t = _NONE, 0
            if i and j and up[c] > _NONE:
                a, b = Q[i - 1], R[j - 1]
                v, t = up[c] + (MATCH if a == b and 0 <= a < 4 else -PENALTY), 0
            if i and c + 1 <= 2 * B and up[c + 1] > _NONE and up[c + 1] - PENALTY > v:
                v, t = up[c + 1] - PENALTY, 1
            if j and c and row[c - 1] > _NONE and row[c - 1] - PENALTY > v:
                v, t = row[c - 1] - PENALTY, 2
            if v == _NONE:
                continue
            row[c], trow[c] = v, t
            if (v, -(i + j), -i) > (best[0], -best[1], -best[2]):
                best = (v, i + j, i, j)
    score, _, i, j = best
    ei, ej = i, j
    ops = []
    while i or j:
        t = T[i][j - i + B]
        if t == 0:
            a, b = Q[i - 1], R[j - 1]
            ops.append("=" if a == b and 0 <= a < 4 else "X")
            i, j = i - 1, j - 1
        elif t == 1:
            ops.append("I")
            i -= 1
        else:
            ops.append("D")
            j -= 1
    return score, ei, ej, "".join(ops)


def run_words(ops):
    """a string over '=XID' -> run words count << 2 | op"""
    out = []
    for o in ops:
        code = "=XID".index(o)
        if out and out[-1] & 3 == code:
            out[-1] += 4
        else:
            out.append(4 | code)
    return out


def tails(q, r, q_pos, r_pos, side):
    """Code arrays of the read on the aligned strand and of the contig, the span's end (side 1: q_en, r_en) or start (side 0: q_st,
    r_st) -> (Q, R), nearest base first"""
    if side:
        Q = q[q_pos:min(len(q), q_pos + EXT_MAX)]
        R = r[r_pos:min(len(r), r_pos + len(Q) + EXT_BAND)]
        return [int(x) for x in Q], [int(x) for x in R]
    Q = q[max(0, q_pos - EXT_MAX):q_pos][::-1]
    R = r[max(0, r_pos - len(Q) - EXT_BAND):r_pos][::-1]
    return [int(x) for x in Q], [int(x) for x in R]


def extend_end(q, r, q_pos, r_pos, side):
    """-> (score, query bases, reference bases, run words in read order)"""
    score, i, j, back = extend(*tails(q, r, q_pos, r_pos, side))
    return score, i, j, run_words(back if side == 0 else back[::-1])


def merge_cigar(cigar, words):
    """append run words (= X I D) to a [(count, op)] CIGAR over M I D, merging equal neighbours"""
    for w in words:
        cnt, op = w >> 2, (0, 0, 1, 2)[w & 3]
        if cigar and cigar[-1][1] == op:
            cigar[-1] = (cigar[-1][0] + cnt, op)
        else:
            cigar.append((cnt, op))
    return cigar


def map_anchors(anchors, seq, index, max_dist=5000, bandwidth=500, min_cnt=3, min_score=40):
    """mapper_ref.map_anchors with both ends extended"""
    k = index.k
    idx, s1, s2 = M.chain(anchors, k, max_dist, bandwidth)
    if len(idx) < min_cnt or s1 < min_score:
        return None
    st, ci = anchors[idx[0]][:2]
    ca = [(anchors[i][2], anchors[i][3]) for i in idx]
    q = M.codes(M.revcomp(seq) if st else seq)
    r = M.codes(index.seqs[ci])
    q_st, q_en, r_st, r_en, pieces = M.span_and_pieces(ca, k, q, r)
    qa, ra = M.np.where(q > 3, 0, q), M.np.where(r > 3, 0, r)
    _, li, lj, lruns = extend_end(q, r, q_st, r_st, 0)
    _, ri, rj, rruns = extend_end(q, r, q_en, r_en, 1)
    cigar = merge_cigar([], lruns)
    for q0, q1, r0, r1 in pieces:
        merge_cigar(cigar, [(cnt << 2) | "=XID".index(o) for cnt, o in M.nw_ops(qa[q0:q1], ra[r0:r1])])
    merge_cigar(cigar, rruns)
    q_st, q_en, r_st, r_en = q_st - li, q_en + ri, r_st - lj, r_en + rj
    nm, md, mlen, blen = M.finish(cigar, q, r, q_st, r_st)
    if st:
        q_st, q_en = len(q) - q_en, len(q) - q_st
    return dict(ctg=index.names[ci], r_st=r_st, r_en=r_en, q_st=q_st, q_en=q_en, strand=-1 if st else 1,
                mapq=M.mapq_of(s1, s2, len(idx)), cigar=[(c, o) for c, o in cigar],
                cigar_str="".join("%d%s" % (c, "MID"[o]) for c, o in cigar), NM=nm, MD=md, mlen=mlen, blen=blen)


def map_read(seq, index, **chain_kw):
    seq = seq.upper()
    return map_anchors(M.seed(M.sketch(seq, index.k, index.w), len(seq), index), seq, index, **chain_kw)

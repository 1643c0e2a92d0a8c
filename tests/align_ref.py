"""Plain restatement of the Smith-Waterman definition of DESIGN.md section 6 (full matrices, the traceback exactly as worded), used by
tests/test_align_cpu.py and tests/test_gpu_align.py. The fill is vectorised over anti-diagonals so that one 4096 x 4096 case is
affordable; the traceback compares matrix VALUES (it keeps no direction bits, unlike the kernel).

    E(i,j) = max(H(i,j-1) - open, E(i,j-1) - extend)        deletion: consumes a ref base   (D)
    F(i,j) = max(H(i-1,j) - open, F(i-1,j) - extend)        insertion: consumes a seq base  (I)
    H(i,j) = max(0, H(i-1,j-1) + s(seq_i, ref_j), E(i,j), F(i,j))      H(0,.) = H(.,0) = 0, E and F start at -infinity

End cell: the largest H, among equals the smallest i, then the smallest j. In H: stop at H = 0, otherwise prefer the diagonal, then E,
then F. In E / F: when opening and extending give the same value, take the open (return to H).
"""
import numpy as np

NEG = -(1 << 40)                                  # "-infinity" in int64: no sum of scores comes near it
DEFAULT = (5, -4, 8, 4)                           # match, mismatch, gap_open, gap_extend
COLUMNS = ("score", "num_correct", "num_mismatches", "num_insertions", "num_deletions",
           "align_ref_start", "align_ref_end", "align_seq_start", "align_seq_end", "num_runs")
EMPTY = [0, 0, 0, 0, 0, 0, -1, 0, -1, 0]


def _codes(s):
    return np.frombuffer(s.encode() if isinstance(s, str) else bytes(s), np.uint8).astype(np.int64)


def fill(seq, ref, match=5, mismatch=-4, gap_open=8, gap_extend=4):
    """-> H, E, F as int64 [m + 1, n + 1] (row i = seq base i, 1-based; column j = ref base j)."""
    a, b = _codes(seq), _codes(ref)
    m, n = len(a), len(b)
    H = np.zeros((m + 1, n + 1), np.int64)
    E = np.full((m + 1, n + 1), NEG, np.int64)
    F = np.full((m + 1, n + 1), NEG, np.int64)
    for d in range(2, m + n + 1):                 # cells with i + j = d depend on the diagonals d - 1 and d - 2 only
        i = np.arange(max(1, d - n), min(m, d - 1) + 1)
        j = d - i
        s = np.where(a[i - 1] == b[j - 1], match, mismatch)
        e = np.maximum(H[i, j - 1] - gap_open, E[i, j - 1] - gap_extend)
        f = np.maximum(H[i - 1, j] - gap_open, F[i - 1, j] - gap_extend)
        E[i, j], F[i, j] = e, f
        H[i, j] = np.maximum(np.maximum(0, H[i - 1, j - 1] + s), np.maximum(e, f))
    return H, E, F


def sw(seq, ref, match=5, mismatch=-4, gap_open=8, gap_extend=4):
    """-> (the ten integers of COLUMNS, CIGAR string with the ops = X I D)."""
    m, n = len(seq), len(ref)
    if m == 0 or n == 0:
        return list(EMPTY), ""
    H, E, F = fill(seq, ref, match, mismatch, gap_open, gap_extend)
    flat = int(np.argmax(H[1:, 1:]))              # the first maximum in row-major order: the smallest i, then the smallest j
    i, j = flat // n + 1, flat % n + 1
    score = int(H[i, j])
    if score == 0:
        return list(EMPTY), ""
    end_i, end_j = i, j
    ops, state = [], "H"
    while True:
        if state == "H":
            if H[i, j] == 0:
                break
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
    ops.reverse()
    cigar = compress(ops)
    cnt = {c: ops.count(c) for c in "=XID"}
    return [score, cnt["="], cnt["X"], cnt["I"], cnt["D"], j, end_j - 1, i, end_i - 1, len(parse(cigar))], cigar


def compress(ops):
    out, k = [], 0
    while k < len(ops):
        e = k
        while e < len(ops) and ops[e] == ops[k]:
            e += 1
        out.append("%d%s" % (e - k, ops[k]))
        k = e
    return "".join(out)


def parse(cigar):
    """'3=1X' -> [(3, '='), (1, 'X')]"""
    out, num = [], ""
    for ch in cigar:
        if ch.isdigit():
            num += ch
        else:
            out.append((int(num), ch))
            num = ""
    assert num == ""
    return out


def replay(cigar, seq, ref, seq_start, ref_start, match=5, mismatch=-4, gap_open=8, gap_extend=4):
    """Walk a CIGAR over the two strings from the given starts -> (score by the four parameters, seq_end, ref_end inclusive, counts).
    Asserts that '=' sits on equal bases and 'X' on unequal ones. Independent of the matrices."""
    i, j, score = seq_start, ref_start, 0
    cnt = {c: 0 for c in "=XID"}
    for k, op in parse(cigar):
        assert k > 0
        cnt[op] += k
        if op in "=X":
            for _ in range(k):
                assert (seq[i] == ref[j]) == (op == "="), (op, i, j)
                i, j = i + 1, j + 1
            score += k * (match if op == "=" else mismatch)
        elif op == "I":
            i += k
            score -= gap_open + (k - 1) * gap_extend
        else:
            assert op == "D"
            j += k
            score -= gap_open + (k - 1) * gap_extend
    return score, i - 1, j - 1, cnt


def random_seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, size=n))


def planted(rng, length, n_sub, n_ins, n_del):
    """A random reference of `length` bases and a copy with isolated edits: substitutions, single-base insertions and single-base
    deletions, at least 25 bases apart and at least 20 from either end -> (seq, ref). An isolated substitution costs 9 against a
    perfect match while any detour through gaps costs at least 16; a length difference of one needs a gap, and one gap of length one
    with no mismatch is the cheapest way: the optimal alignment has exactly the planted counts."""
    total = n_sub + n_ins + n_del
    assert 40 + 25 * max(total - 1, 0) <= length - 1
    ref = rng.integers(0, 4, size=length)
    slack = length - 41 - 25 * max(total - 1, 0)
    gaps = np.sort(rng.integers(0, slack + 1, size=total))
    pos = 20 + gaps + 25 * np.arange(total)
    kinds = rng.permutation(["S"] * n_sub + ["I"] * n_ins + ["D"] * n_del)
    out, last = [], 0
    for p, kind in zip(pos, kinds):
        out.extend(ref[last:p])
        if kind == "S":
            out.append((ref[p] + rng.integers(1, 4)) % 4)
            last = p + 1
        elif kind == "I":
            out.append(rng.integers(0, 4))
            last = p
        else:
            last = p + 1
    out.extend(ref[last:])
    return "".join("ACGT"[c] for c in out), "".join("ACGT"[c] for c in ref)

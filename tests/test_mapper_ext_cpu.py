"""The end extension's definition (tests/mapper_ext_ref.py) against a full-matrix evaluation of its rules written separately here,
its stated corner cases, and its records on the planted read set. No GPU."""
import random

import numpy as np
import pytest

import mapper_cases as cases
import mapper_ext_ref as X
import mapper_ref as M


def full_dp(Q, R, band=None):
    """The recurrence over the whole matrix (band=None) or with the cells |j - i| > band absent, the end cell by sorting, and the path
    re-derived from the VALUES (no stored directions) -> (score, i, j, ops from the end cell back to (0,0))."""
    m, n = len(Q), len(R)
    S = {}
    for i in range(m + 1):
        for j in range(n + 1):
            if band is not None and abs(j - i) > band:
                continue
            if i == 0 and j == 0:
                S[0, 0] = 0
                continue
            cand = []
            if (i - 1, j - 1) in S:
                cand.append(S[i - 1, j - 1] + (2 if Q[i - 1] == R[j - 1] and Q[i - 1] in (0, 1, 2, 3) else -4))
            if (i - 1, j) in S:
                cand.append(S[i - 1, j] - 4)
            if (i, j - 1) in S:
                cand.append(S[i, j - 1] - 4)
            if cand:
                S[i, j] = max(cand)
    score, _, i, j = min((-v, i + j, i, j) for (i, j), v in S.items())[0:4]
    score = -score
    end = (i, j)
    ops = []
    while (i, j) != (0, 0):
        v = S[i, j]
        match = i and j and Q[i - 1] == R[j - 1] and Q[i - 1] in (0, 1, 2, 3)
        if (i - 1, j - 1) in S and v == S[i - 1, j - 1] + (2 if match else -4):
            ops.append("=" if match else "X")
            i, j = i - 1, j - 1
        elif (i - 1, j) in S and v == S[i - 1, j] - 4:
            ops.append("I")
            i -= 1
        else:
            assert (i, j - 1) in S and v == S[i, j - 1] - 4
            ops.append("D")
            j -= 1
    return score, end[0], end[1], "".join(ops)


def c(text):
    return [int(x) for x in M.codes(text)]


def test_banded_restatement_equals_the_full_matrix_on_low_divergence_tails():
    rng = random.Random(41)
    extended = 0
    for case in range(200):
        length = rng.randint(0, 120)
        tail = cases.random_seq(rng, length)
        ref = cases.mutate(rng, tail, 0.06) + cases.random_seq(rng, X.EXT_BAND)
        Q, R = c(tail), c(ref)[:length + X.EXT_BAND]
        got = X.extend(Q, R)
        assert got == full_dp(Q, R), (case, tail, ref)
        assert got == full_dp(Q, R, band=X.EXT_BAND)
        assert got[0] == 2 * got[3].count("=") - 4 * (len(got[3]) - got[3].count("="))
        assert got[1] == len(got[3]) - got[3].count("D") and got[2] == len(got[3]) - got[3].count("I")
        extended += got[0] > 0
    assert extended > 150                                                # most of these tails are worth extending


def test_stated_corner_cases():
    # a mismatch and two matches gain nothing: not taken; three matches are
    assert X.extend(c("TAC"), c("GAC")) == (0, 0, 0, "")
    assert X.extend(c("TACG"), c("GACG")) == (2, 4, 4, "===X")
    # the smallest i + j among equal scores: the fourth match would be paid for by the mismatch before it
    assert X.extend(c("ACGTAC"), c("ACGAAC")) == (6, 3, 3, "===")
    # only mismatches
    assert X.extend(c("AAAA"), c("CCCC")) == (0, 0, 0, "")
    # a base outside ACGT matches nothing, not even itself
    assert X.extend(c("ACNGT"), c("ACNGT")) == (4, 2, 2, "==")
    assert X.extend(c("ACGTNACGTA"), c("ACGTNACGTA")) == (14, 10, 10, "=====X====")
    assert X.extend(c("ACGTNACGTA"), c("ACGTCACGTA"))[:3] == (14, 10, 10) and X.extend(c("ACGTCACGTA"), c("ACGTNACGTA"))[:3] == (14, 10, 10)
    # empty tails
    assert X.extend([], c("ACGT")) == (0, 0, 0, "") and X.extend(c("ACGT"), []) == (0, 0, 0, "") and X.extend([], []) == (0, 0, 0, "")
    # the path's preference where a value has several explanations: diagonal, then I, then D
    assert X.extend(c("AACCC"), c("ACCC")) == full_dp(c("AACCC"), c("ACCC"))
    assert X.run_words("===XIID") == [(3 << 2) | 0, (1 << 2) | 1, (2 << 2) | 2, (1 << 2) | 3]


@pytest.mark.parametrize("gap,bridged", [(32, True), (33, False)])
def test_a_gap_of_the_band_is_bridged_and_one_more_is_not(gap, bridged):
    rng = random.Random(gap)
    unit = "".join(rng.choice("ACT") for _ in range(100))
    # D: the reference holds `gap` bases the read lacks (G never occurs in the read)
    Q, R = c(unit), c("G" * gap + unit)[:100 + X.EXT_BAND]
    got = X.extend(Q, R)
    assert got == full_dp(Q, R, band=X.EXT_BAND)
    if bridged:
        assert got == (200 - 4 * 32, 100, 132, "=" * 100 + "D" * 32) and got == full_dp(Q, R)
    else:
        assert got[0] < 200 - 4 * 33 and got[2] - got[1] <= X.EXT_BAND
    # I: the read holds `gap` bases the reference lacks
    Q, R = c("G" * gap + unit), c(unit)
    got = X.extend(Q, R)
    assert got == full_dp(Q, R, band=X.EXT_BAND)
    if bridged:
        assert got == (200 - 4 * 32, 132, 100, "=" * 100 + "I" * 32) and got == full_dp(Q, R)
    else:
        assert got[0] < 200 - 4 * 33 and got[1] - got[2] <= X.EXT_BAND
        assert full_dp(Q, R)[0] == 200 - 4 * 33                          # the full matrix does bridge it: the band is what binds


def test_tails_stop_at_the_read_and_the_contig():
    q, r = M.codes("ACGTACGTAC" * 80), M.codes("ACGTACGTAC" * 80)
    Q, R = X.tails(q, r, 100, 100, 1)
    assert len(Q) == X.EXT_MAX and len(R) == X.EXT_MAX + X.EXT_BAND and Q[:3] == c("ACG")
    Q, R = X.tails(q, r, 790, 795, 1)                                    # ten read bases left, five of the contig
    assert len(Q) == 10 and len(R) == 5
    assert X.extend_end(q, r, 790, 795, 1)[:3] == X.extend(Q, R)[:3]
    Q, R = X.tails(q, r, 600, 3, 0)                                      # the contig starts three bases to the left
    assert len(Q) == X.EXT_MAX and R == c("ACG")[::-1] and Q[:2] == [int(q[599]), int(q[598])]
    assert X.tails(q, r, 0, 50, 0) == ([], c("ACGTACGTAC" * 5)[::-1][:X.EXT_BAND])
    assert X.tails(q, r, 800, 800, 1) == ([], []) and X.tails(q, r, 10, 0, 0)[1] == []
    # a reference tail cut short by the contig end: the extension uses what is there
    read, contig = "ACGTTGCAAGGCTTAACCGA", "ACGTTGCAAGGC"
    score, i, j, words = X.extend_end(M.codes(read), M.codes(contig), 4, 4, 1)
    assert (score, i, j, words) == (16, 8, 8, [(8 << 2) | 0])
    # the left end's runs come in read order
    score, i, j, words = X.extend_end(M.codes("TTACGAACGT"), M.codes("GGGGTTACGTACGT"), 6, 10, 0)
    assert (score, i, j) == (2 * 5 - 4, 6, 6) and words == [(5 << 2) | 0, (1 << 2) | 1]


@pytest.fixture(scope="module")
def planted_extended():
    contigs, reads = cases.planted()
    index = M.Index(contigs)
    return contigs, reads, [X.map_read(r[0], index) for r in reads]


def test_extended_records_replay_and_reach_further(planted_extended):
    contigs, reads, got = planted_extended
    plain = cases.planted_expected()
    by_name = dict(contigs)
    both_ends = both_ends_plain = 0
    for (seq, _ci, _strand, _s, _e), rec, old in zip(reads, got, plain):
        assert (rec is None) == (old is None)
        if rec is None:
            continue
        cases.check_replay(rec, seq, by_name[rec["ctg"]])
        assert rec["q_st"] <= old["q_st"] and rec["q_en"] >= old["q_en"] and rec["r_st"] <= old["r_st"] and rec["r_en"] >= old["r_en"]
        assert (rec["ctg"], rec["strand"], rec["mapq"]) == (old["ctg"], old["strand"], old["mapq"])
        both_ends += rec["q_st"] == 0 and rec["q_en"] == len(seq)
        both_ends_plain += old["q_st"] == 0 and old["q_en"] == len(seq)
    assert both_ends > both_ends_plain and both_ends >= len(reads) // 2


def test_a_substitution_near_the_end_is_crossed_only_with_the_extension():
    rng = random.Random(9)
    contig = cases.random_seq(rng, 4000)
    read = contig[1000:1600]
    read = read[:-6] + ("A" if read[-6] != "A" else "C") + read[-5:]      # the substitution has five bases behind it
    index = M.Index([("c", contig)])
    old, new = M.map_read(read, index), X.map_read(read, index)
    assert old["q_en"] == len(read) - 6 and new["q_en"] == len(read) and new["r_en"] == 1600 and new["NM"] == old["NM"] + 1
    cases.check_replay(new, read, contig)
    rc_old, rc_new = M.map_read(M.revcomp(read), index), X.map_read(M.revcomp(read), index)
    assert rc_old["q_st"] == 6 and rc_new["q_st"] == 0 and rc_new["q_en"] == len(read) and rc_new["strand"] == -1
    assert (rc_new["r_st"], rc_new["r_en"], rc_new["cigar_str"]) == (new["r_st"], new["r_en"], new["cigar_str"])
    cases.check_replay(rc_new, M.revcomp(read), contig)
    assert np.array_equal(M.codes(read), M.codes(M.revcomp(M.revcomp(read))))

"""Duplex calling without a GPU: the restatements of tests/duplex_ref.py against exhaustive enumeration and planted edits, the
pipeline restatement and the host functions of bonito_amd/duplex.py against the reference's own outputs
(tests/golden/duplex_cases.json, written by tests/golden/make_golden_duplex.py), and the command line's parsers."""
import itertools
import json
import os

import numpy as np
import pytest

import align_ref as ar
import duplex_ref as dr
from bonito_amd import duplex
from bonito_amd.cli import duplex as cli

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "duplex_cases.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)["cases"]


def words(alphabet, longest):
    return ["".join(w) for k in range(longest + 1) for w in itertools.product(alphabet, repeat=k)]


# ---- global alignment ----------------------------------------------------------------------------------------------------------

def nw_paths(seq, ref):
    """Every alignment of the two strings as (cost, op string), by the three moves of the recurrence."""
    def walk(i, j):
        if i == 0 and j == 0:
            yield 0, ""
        if i > 0 and j > 0:
            for c, p in walk(i - 1, j - 1):
                yield c + (seq[i - 1] != ref[j - 1]), p + ("=" if seq[i - 1] == ref[j - 1] else "X")
        if j > 0:
            for c, p in walk(i, j - 1):
                yield c + 1, p + "D"
        if i > 0:
            for c, p in walk(i - 1, j):
                yield c + 1, p + "I"
    return list(walk(len(seq), len(ref)))


def preferred(paths, best):
    """Of the paths with the best value the one the preference order selects, walking back from the end: a diagonal move before D
    before I at every step."""
    rank = {"=": 0, "X": 0, "D": 1, "I": 2}
    return min((p for c, p in paths if c == best), key=lambda p: [rank[o] for o in reversed(p)])


def test_nw_restatement_against_exhaustive_enumeration():
    for seq in words("AC", 4):
        for ref in words("AC", 4):
            paths = nw_paths(seq, ref)
            best = min(c for c, _ in paths)
            row, cigar = dr.nw(seq, ref)
            path = preferred(paths, best)
            assert row[0] == best == dr.edit_distance(seq, ref), (seq, ref)
            assert cigar == ar.compress(list(path)), (seq, ref)
            assert row[1:5] == [path.count(c) for c in "=XID"] and row[5] == len(ar.parse(cigar))


def test_nw_restatement_empty_inputs():
    assert dr.nw("", "") == ([0, 0, 0, 0, 0, 0], "")
    assert dr.nw("ACG", "") == ([3, 0, 0, 3, 0, 1], "3I")
    assert dr.nw("", "AC") == ([2, 0, 0, 0, 2, 1], "2D")


def test_nw_planted_edits_give_exactly_their_distance():
    rng = np.random.default_rng(31)
    for _ in range(12):
        length = int(rng.integers(270, 401))                                # nine edits 25 apart need 241 bases
        counts = [int(v) for v in rng.integers(0, 4, size=3)]
        seq, ref = ar.planted(rng, length, *counts)
        row, cigar = dr.nw(seq, ref)
        assert row[0] == sum(counts) == dr.edit_distance(seq, ref)
        assert row[2:5] == counts                                           # substitutions, insertions, deletions: isolated
        assert dr.lengths(ar.parse(cigar)) == (len(seq), len(ref))


# ---- semi-global alignment ---------------------------------------------------------------------------------------------------------

def sg_paths(seq, ref, match, mismatch, gap_open, gap_extend):
    """Every semi-global alignment as (score, end cell, start cell, op string of the aligned part): a start on row 0 or column 0, an
    end on the last row or the last column, moves as in the recurrences (a gap of k costs open + (k - 1) * extend)."""
    m, n = len(seq), len(ref)
    out = []

    def walk(i, j, score, ops, start):
        if (i == m or j == n) and ops:
            out.append((score, (i, j), start, ops))
        if i < m and j < n:
            eq = seq[i] == ref[j]
            walk(i + 1, j + 1, score + (match if eq else mismatch), ops + ("=" if eq else "X"), start)
        if j < n and i > 0:                                                 # a D run inside the alignment (row 0 is free instead)
            cost = gap_extend if ops.endswith("D") else gap_open
            walk(i, j + 1, score - cost, ops + "D", start)
        if i < m and j > 0:
            cost = gap_extend if ops.endswith("I") else gap_open
            walk(i + 1, j, score - cost, ops + "I", start)

    for i in range(m + 1):
        for j in range(n + 1):
            if i == 0 or j == 0:
                walk(i, j, 0, "", (i, j))
    return out


def test_sg_restatement_against_exhaustive_enumeration():
    scoring = dr.SG_DEFAULT
    for seq in words("AC", 3)[1:]:
        for ref in words("AC", 4)[1:]:
            m, n = len(seq), len(ref)
            paths = sg_paths(seq, ref, *scoring)
            best = max(p[0] for p in paths)
            row, cigar = dr.sg(seq, ref, *scoring)
            assert row[0] == best, (seq, ref)
            ops = ar.parse(cigar)
            assert dr.lengths(ops) == (m, n)                                # the CIGAR spans both sequences
            # the end cell: among the best the smallest i, then the smallest j
            end = min(p[1] for p in paths if p[0] == best)
            assert (row[8] + 1, row[6] + 1) == end, (seq, ref)
            # the reported path is one of the enumerated best ones with this end, and rescoring it gives the score
            start = (row[7], row[5])
            inner = "".join(c * k for k, c in ops)
            inner = inner[start[0] + start[1]:len(inner) - (m - end[0]) - (n - end[1])]
            assert (best, end, start, inner) in paths, (seq, ref, cigar)
            # the preference order, walking back: the diagonal, then E (D), then F (I)
            rank = {"=": 0, "X": 0, "D": 1, "I": 2}
            same_end = [p for p in paths if p[0] == best and p[1] == end]
            first = min(same_end, key=lambda p: [rank[o] for o in reversed(p[3])])
            assert inner == first[3], (seq, ref, cigar)


def test_sg_restatement_overhangs_and_empty_inputs():
    assert dr.sg("", "") == ([0, 0, 0, 0, 0, 0, -1, 0, -1, 0], "")
    assert dr.sg("ACG", "")[1] == "3I" and dr.sg("", "AC")[1] == "2D"
    rng = np.random.default_rng(32)
    ref = ar.random_seq(rng, 200)
    row, cigar = dr.sg(ref[50:120], ref)
    assert cigar == "50D70=80D" and row[:5] == [350, 70, 0, 0, 130] and row[5:9] == [50, 119, 0, 69]
    row, cigar = dr.sg(ref[100:] + "ACGTACGTAC", "TTTTT" + ref[:160])          # the query's head on the reference's tail
    assert row[0] == 300 and dr.lengths(ar.parse(cigar)) == (110, 165) and "60=" in cigar


# ---- the pipeline against the reference's own outputs ------------------------------------------------------------------------------

class Restated:
    """The two aligners of the pipeline by their restatements"""

    def nw(self, queries, refs):
        return [dr.nw(q, r)[1] for q, r in zip(queries, refs)]

    def sg(self, queries, refs):
        return [dr.sg(q, r, *dr.SG_DEFAULT)[1] for q, r in zip(queries, refs)]


def phred(qstring):
    return np.frombuffer(qstring.encode(), np.uint8) - np.uint8(33)


def test_fixture_covers_the_cases(golden):
    names = {c["name"] for c in golden}
    assert {"no_long_match", "identical", "ties", "homopolymers", "short_identical"} <= names
    assert any(c["sequence"] == "" for c in golden) and any(c["cigar"].split("=")[0].isdigit() for c in golden)
    assert any(c["cigar"] != c["nw_cigar"] for c in golden)                 # the end repair does change alignments


def test_adjusted_scores_equal_the_reference(golden):
    for c in golden:
        for seq, q, shift, want in ((c["temp_seq"], c["temp_qstring"], 1, c["adj_temp"]), (c["comp_seq"], c["comp_qstring"], -1, c["adj_comp"])):
            want = np.array(want, np.float32)
            for got in (dr.adj_qscores(phred(q), seq, shift), duplex.adjust_qscores(phred(q), seq, shift)):
                assert got.dtype == np.float32 and got.tobytes() == want.tobytes(), c["name"]


def test_alignment_glue_trim_and_lengths_equal_the_reference(golden):
    for c in golden:
        ref = duplex.revcomp(c["comp_seq"])
        assert ref == dr.revcomp(c["comp_seq"])
        want = ar.parse(c["cigar"])
        assert dr.adj_align(c["temp_seq"], ref) == want, c["name"]
        assert duplex.adj_align([c["temp_seq"]], [ref], aligners=Restated()) == [[(k, o) for k, o in want]], c["name"]
        assert list(dr.lengths(want)) == c["seq_lens"] == list(duplex.lengths(duplex.parse_cigar(c["cigar"])))
        (head, ts, cs), (both, te, ce) = c["trim_start"], c["trim_end"]
        for trim in (dr.trim, duplex.trim):
            ops, a, b, e, f = trim(duplex.parse_cigar(c["cigar"]))
            assert ops == duplex.parse_cigar(both) and (a, b) == (ts, cs), c["name"]
            if both:
                assert (e, f) == (te, ce), c["name"]


def test_consensus_equals_the_reference(golden):
    for c in golden:
        if "consensus" not in c:
            continue
        ref = dr.revcomp(c["comp_seq"])
        (_, ts, cs), (both, te, ce) = c["trim_start"], c["trim_end"]
        t, tq = c["temp_seq"], np.array(c["adj_temp"], np.float32)
        cq = np.array(c["adj_comp"], np.float32)[::-1]
        args = (t[ts:len(t) - te], tq[ts:len(t) - te], ref[cs:len(ref) - ce], cq[cs:len(ref) - ce])
        assert list(dr.consensus(ar.parse(both), *args)) == c["consensus"], c["name"]
        assert list(duplex.consensus(duplex.parse_cigar(both), *args)) == c["consensus"], c["name"]


def test_whole_pipeline_equals_the_reference(golden):
    for c in golden:
        got = dr.call_pair(c["temp_seq"], phred(c["temp_qstring"]), c["comp_seq"], phred(c["comp_qstring"]))
        assert got == (c["sequence"], c["qstring"]), c["name"]
    stats = {}
    got = duplex.call_pairs([c["temp_seq"] for c in golden], [c["temp_qstring"] for c in golden], [c["comp_seq"] for c in golden],
                            [c["comp_qstring"] for c in golden], aligners=Restated(), stats=stats)
    assert got == [(c["sequence"], c["qstring"]) for c in golden]
    assert stats == {"unaligned": 0, "kept_nw": 0}


def test_ends_over_the_semi_global_limit_keep_their_global_cigar():
    class Fake:
        def __init__(self):
            self.sg_calls = []

        def nw(self, queries, refs):
            return ["5000X20=5000X", "30X", None]

        def sg(self, queries, refs):
            self.sg_calls.append(list(zip(queries, refs)))
            return ["30X"] * len(queries)

    fake, stats = Fake(), {}
    got = duplex.adj_align(["A" * 10020, "A" * 30, "A" * 7], ["C" * 10020, "C" * 30, "C" * 7], aligners=fake, stats=stats)
    assert got == [[(5000, "X"), (20, "="), (5000, "X")], [(30, "X")], None]
    assert stats == {"kept_nw": 2, "unaligned": 1} and fake.sg_calls == [[("A" * 30, "C" * 30)]]
    fake, stats = Fake(), {}
    fake.nw = lambda q, r: ["5000X"]
    assert duplex.adj_align(["A" * 5000], ["C" * 5000], aligners=fake, stats=stats) == [None] and stats["unaligned"] == 1


# ---- the command line ----------------------------------------------------------------------------------------------------------

def test_read_calls_fastq_and_sam(tmp_path):
    fq = tmp_path / "calls.fastq"
    fq.write_text("@r1 qs:f:12.00\tns:i:5\nACGT\n+\n!!5I\n@r2\nAC\n+\nII\n@r1\nTTTT\n+\nIIII\n\n")
    assert cli.read_calls(str(fq)) == {"r1": ("ACGT", "!!5I"), "r2": ("AC", "II")}
    sam = tmp_path / "calls.sam"
    sam.write_text("@HD\tVN:1.5\tSO:unknown\n@PG\tID:basecaller\tPN:bonito_amd\n"
                   "r1\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t!!5I\tNM:i:0\tqs:f:3.1\n"
                   "r1\t4\t*\t0\t0\t*\t*\t0\t0\tTTTT\tIIII\tNM:i:0\n"
                   "r3\t2308\t*\t0\t0\t*\t*\t0\t0\tGG\tII\n"
                   "r2\t4\t*\t0\t0\t*\t*\t0\t0\tAC\t*\n")
    assert cli.read_calls(str(sam)) == {"r1": ("ACGT", "!!5I"), "r2": ("AC", "!!")}
    bad = tmp_path / "bad.fastq"
    bad.write_text("@r1\nACGT\n+\n!!\n")
    with pytest.raises(ValueError, match="FASTQ"):
        cli.read_calls(str(bad))
    empty = tmp_path / "empty.fastq"
    empty.write_text("")
    assert cli.read_calls(str(empty)) == {}


def test_read_pairs_and_arguments(tmp_path):
    path = tmp_path / "pairs.txt"
    path.write_text("template complement\na b\nc\td\n\n")
    assert cli.read_pairs(str(path)) == [("a", "b"), ("c", "d")]
    assert cli.read_pairs(str(path), header=False)[0] == ("template", "complement")
    args = cli.argparser().parse_args(["calls.fastq", "pairs.txt", "--no-header", "--min-qscore", "12", "--batch", "64"])
    assert (args.calls, args.duplex_pairs_file, args.no_header, args.min_qscore, args.device, args.batch) == \
        ("calls.fastq", "pairs.txt", True, 12, "cuda", 64)
    assert not cli.argparser().parse_args(["a", "b"]).no_header and "pysam" in cli.argparser().description
    from bonito_amd import __main__ as entry
    assert "duplex" in entry.modules

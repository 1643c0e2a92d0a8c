"""Smith-Waterman alignment without a GPU: the restatement (tests/align_ref.py) against an exhaustive enumeration and against planted
edits; util.accuracy / cigar_to_sam / the evaluate report on hand-made results; the new ABI symbols and their argument errors."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import align_ref as ar


def _all_alignment_scores(seq, ref, match, mismatch, gap_open, gap_extend):
    """The best score over EVERY local alignment, by enumeration: every start cell, every string of ops (diagonal, I, D) that stays
    inside the two strings, rescored run by run. No dynamic programming."""
    best = 0

    def walk(i, j, ops):
        nonlocal best
        if ops:
            score, k = 0, 0
            while k < len(ops):
                e = k
                while e < len(ops) and ops[e][0] == ops[k][0]:
                    e += 1
                if ops[k][0] == "M":
                    score += sum(match if o[1] else mismatch for o in ops[k:e])
                else:
                    score -= gap_open + (e - k - 1) * gap_extend
                k = e
            best = max(best, score)
        if i < len(seq) and j < len(ref):
            walk(i + 1, j + 1, ops + [("M", seq[i] == ref[j])])
        if i < len(seq):
            walk(i + 1, j, ops + [("I", None)])
        if j < len(ref):
            walk(i, j + 1, ops + [("D", None)])

    for i in range(len(seq)):
        for j in range(len(ref)):
            walk(i, j, [])
    return best


@pytest.mark.parametrize("params", [ar.DEFAULT, (2, -3, 5, 2), (3, -1, 2, 1)])
def test_restatement_score_equals_exhaustive_enumeration(params):
    words = ["".join(w) for k in range(0, 5) for w in itertools.product("AC", repeat=k)]
    for seq in words:
        for ref in words:
            if len(seq) + len(ref) > 7:
                continue
            row, cigar = ar.sw(seq, ref, *params)
            assert row[0] == _all_alignment_scores(seq, ref, *params), (seq, ref)
            if row[0]:
                score, se, re_, cnt = ar.replay(cigar, seq, ref, row[7], row[5], *params)
                assert (score, se, re_) == (row[0], row[8], row[6])
            else:
                assert row == ar.EMPTY and cigar == ""


def test_restatement_tie_breaks_as_worded():
    # two equal maxima: the smaller i wins, then the smaller j
    row, cigar = ar.sw("ACGTTTTACG", "ACG")
    assert row[0] == 15 and (row[7], row[8], row[5], row[6]) == (0, 2, 0, 2) and cigar == "3="
    row, _ = ar.sw("ACG", "ACGTTTTACG")
    assert (row[7], row[8], row[5], row[6]) == (0, 2, 0, 2)
    # one base repeated: the diagonal is preferred everywhere, so the alignment is the main diagonal ending at the first full-score cell
    row, cigar = ar.sw("AAAA", "AAAAAA")
    assert row[0] == 20 and cigar == "4=" and (row[5], row[6]) == (0, 3)
    assert ar.sw("", "ACGT") == (ar.EMPTY, "") and ar.sw("AAAA", "CCCC") == (ar.EMPTY, "")
    # a gap of length k costs open + (k - 1) * extend: 20 matches, a 3-base deletion (8 + 4 + 4), 20 matches
    a, b = "ACGTTGCAAGGCTTACCGAT", "GGATCCTTAGACCAGTTGCA"
    row, cigar = ar.sw(a + b, a + "CCC" + b)
    assert row[0] == 200 - 16 and cigar == "20=3D20=" and row[1:5] == [40, 0, 0, 3]
    assert ar.COLUMNS[9] == "num_runs" and row[9] == 3


def _planted_cases():
    rng = np.random.default_rng(20240611)
    cases = []
    for k in range(40):
        length = int(rng.integers(150, 401))
        room = (length - 41) // 25 + 1
        total = int(rng.integers(1, min(room, 9) + 1))
        cut = np.sort(rng.integers(0, total + 1, size=2))
        cases.append((length, int(cut[0]), int(cut[1] - cut[0]), int(total - cut[1]), 1000 + k))
    return cases


@pytest.mark.parametrize("length,n_sub,n_ins,n_del,seed", _planted_cases())
def test_restatement_returns_the_planted_edits(length, n_sub, n_ins, n_del, seed):
    seq, ref = ar.planted(np.random.default_rng(seed), length, n_sub, n_ins, n_del)
    assert len(ref) == length and len(seq) == length + n_ins - n_del
    row, cigar = ar.sw(seq, ref)
    assert row[2:5] == [n_sub, n_ins, n_del], (row, cigar)
    assert row[1] == length - n_sub - n_del
    assert (row[5], row[6], row[7], row[8]) == (0, len(ref) - 1, 0, len(seq) - 1)
    assert all(k == 1 for k, op in ar.parse(cigar) if op in "XID")


def test_accuracy_and_cigar_to_sam_on_hand_made_results():
    from bonito_amd import util
    from bonito_amd.align import AlignResult, SwBatch, accuracy_of, runs_to_cigar
    seq, ref = "TTACGTACGTAA", "GGGACGTTCGTA"
    # seq[2:10] = ACGTACGT against ref[3:11] = ACGTTCGT: 4=1X3=
    r = AlignResult(accuracy=7 / 8, num_correct=7, num_mismatches=1, ref_len=12, seq_len=12, align_ref_start=3, align_ref_end=10,
                    align_seq_start=2, align_seq_end=9, score=31, cigar="4=1X3=")
    assert util.cigar_to_sam(r, seq) == (3, "2S4=1X3=2S")
    assert util.accuracy(ref, seq, result=r) == pytest.approx(87.5)
    assert util.accuracy(ref, seq, min_coverage=0.7, result=r) == 0.0          # 8 columns of 12 reference bases
    assert util.accuracy(ref, seq, min_coverage=0.6, result=r) == pytest.approx(87.5)
    g = AlignResult(num_correct=16, num_mismatches=1, num_insertions=2, num_deletions=1, ref_len=18, seq_len=19, align_ref_start=0,
                    align_ref_end=17, align_seq_start=0, align_seq_end=18, cigar="5=2I6=1X5=1D")
    assert util.cigar_to_sam(g, "A" * 19) == (0, "5=2I6=1X5=1D")
    assert util.accuracy("A" * 18, "A" * 19, result=g) == pytest.approx(100 * 16 / 20)
    assert util.accuracy("A" * 18, "A" * 19, balanced=True, result=g) == pytest.approx(100 * (16 - 2) / 18)
    lead_i = AlignResult(num_correct=4, num_insertions=2, align_ref_start=1, align_ref_end=4, align_seq_start=3, align_seq_end=8,
                         cigar="2I4=")
    assert util.cigar_to_sam(lead_i, "A" * 10) == (1, "5S4=1S")
    lead_d = AlignResult(num_correct=4, num_deletions=2, align_ref_start=1, align_ref_end=6, align_seq_start=3, align_seq_end=6,
                         cigar="2D4=")
    assert util.cigar_to_sam(lead_d, "A" * 7) == (3, "3S4=")
    nothing = AlignResult(ref_len=4, seq_len=0, cigar="")
    assert (nothing.align_ref_end, nothing.align_seq_end, nothing.accuracy) == (-1, -1, 0)
    assert util.cigar_to_sam(nothing, "") == (0, "") and util.accuracy("ACGT", "", result=nothing) == 0.0
    with pytest.raises(ValueError, match="no CIGAR"):
        util.cigar_to_sam(AlignResult(num_correct=1), "A")
    assert runs_to_cigar(np.array([(4 << 2) | 0, (1 << 2) | 1, (2 << 2) | 2, (3 << 2) | 3], np.uint32)) == "4=1X2I3D"
    assert accuracy_of([7, 0], [1, 0], [0, 0], [0, 0]).tolist() == [0.875, 0.0]
    b = SwBatch([[31, 7, 1, 0, 0, 3, 10, 2, 9, 3], [0, 0, 0, 0, 0, 0, -1, 0, -1, 0]], [12, 0], [12, 4], ["4=1X3=", ""])
    assert len(b) == 2 and b[0] == r and b[1] == nothing and b.score.tolist() == [31, 0] and b.accuracy.tolist() == [0.875, 0.0]


def test_evaluate_report_from_arrays():
    from bonito_amd.cli import evaluate
    table = np.array([[440, 90, 5, 2, 3, 1, 98, 0, 96, 9],                    # accuracy 0.9
                      [0, 0, 0, 0, 0, 0, -1, 0, -1, 0],                       # num_correct = 0: a called sequence with nothing in common
                      [0, 0, 0, 0, 0, 0, -1, 0, -1, 0],                       # an empty seq
                      [250, 50, 0, 0, 0, 0, 49, 10, 59, 1]], np.int32)        # accuracy 1.0
    seq_len, ref_len, losses = np.array([100, 7, 0, 60]), np.array([100, 9, 9, 50]), np.array([0.5, 2.0, 3.0, 0.1])
    lines = evaluate.report_lines(table, seq_len, ref_len, losses)
    got = {l[2:18].strip(): l[18:].strip() for l in lines}
    assert got["num_chunks"] == "4" and got["loss mean"] == "1.4000" and got["loss median"] == "1.2500"
    assert got["accuracy"] == "47.50%"                                          # (0.9 + 0 + 0 + 1.0) / 4
    assert got["sub-rate"] == "%.2f%%" % (100 * (5 / 90 + 0) / 2) and got["ins-rate"] == "%.2f%%" % (100 * (2 / 90) / 2)
    assert got["del-rate"] == "%.2f%%" % (100 * (3 / 90) / 2)
    assert got["rates left out"].startswith("2 chunks")
    assert got["seq_len"] == "41.8" and got["seq_lclip"] == "2.5" and got["seq_rclip"] == "%.1f" % ((3 + 7 + 0 + 0) / 4)
    assert got["ref_len"] == "42.0" and got["ref_lclip"] == "0.2" and got["ref_rclip"] == "%.1f" % ((1 + 9 + 9 + 0) / 4)
    assert float(got["accuracy"].rstrip("%")) == 47.5
    summ = evaluate.summ_lines(table, seq_len, ref_len, losses)
    assert summ[0] == "\tloss\taccuracy\tnum_correct\tnum_mismatches\tnum_insertions\tnum_deletions\tref_len\tseq_len\talign_ref_start" \
                      "\talign_ref_end\talign_seq_start\talign_seq_end\n"
    assert summ[1].rstrip("\n").split("\t") == ["0", "0.500000", "0.900000", "90", "5", "2", "3", "100", "100", "1", "98", "0", "96"]
    assert summ[3].rstrip("\n").split("\t") == ["2", "3.000000", "0.000000", "0", "0", "0", "0", "9", "0", "0", "-1", "0", "-1"]
    empty = evaluate.report_lines(np.zeros((0, 10)), [], [], [])
    assert empty[0].endswith(" 0") and "0.00%" in empty[3]
    assert "not computed" not in "\n".join(lines) and "not computed" not in evaluate.argparser().description


def test_symbols_are_declared_bound_and_exported_and_workspace_sizes():
    from bonito_amd import _lib
    text = open(os.path.join(ROOT, "include", "bonito_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = _lib.lib()
    for name in ("bh_sw_workspace", "bh_sw_align"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and hasattr(handle, name)
    assert handle.bh_abi_version() == 1
    head = lambda n: 256 * (-(-8 * n // 256)) + 256 * (-(-16 * n // 256))
    # 4 traceback bits per cell: one dword per lane and step, ceil(seq / 512) passes of ref + 63 steps
    assert handle.bh_sw_workspace(1, 4096, 4096) == head(1) + 2 * 4096 * 8 + 8 * (4096 + 63) * 256
    assert handle.bh_sw_workspace(512, 512, 800) == head(512) + 512 * (800 + 63) * 256      # one pass: no boundary rows
    assert handle.bh_sw_workspace(3, 513, 100) == head(3) + 256 * (-(-3 * 2 * 128 * 8 // 256)) + 3 * 2 * 163 * 256
    assert handle.bh_sw_workspace(2, 0, 0) == head(2)
    for bad in ((0, 10, 10), (-1, 10, 10), (1, 4097, 10), (1, 10, 4097), (1, -1, 10), (1, 10, -1)):
        assert handle.bh_sw_workspace(*bad) == 0, bad


ENTRIES = {"bh_sw_align": (4096, (5, -4, 8, 4)), "bh_sg_align": (4096, (5, -4, 10, 2)), "bh_nw_align": (65536, (64,))}


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_argument_errors_are_raised_before_any_launch(entry):
    """Every call below names pointers that are never dereferenced on the device: the checks run on the host first."""
    from bonito_amd import _lib
    handle = _lib.lib()
    fake = C.c_void_p(4096)
    ip = C.POINTER(C.c_int32)
    limit, default = ENTRIES[entry]
    nw = entry == "bh_nw_align"
    prefix = entry[3:] + ": "

    def workspace(n, s, r):
        return handle.bh_nw_workspace(n, s, r, abs(s - r) + 2 * 64 + 1) if nw else handle.bh_sw_workspace(n, s, r)

    def call(seq_lens, ref_lens, seq_stride=64, ref_stride=64, extra=default, ws_bytes=None, ops=None, ops_stride=0, n=None, n_ops=None):
        sl, rl = np.asarray(seq_lens, np.int32), np.asarray(ref_lens, np.int32)
        n = len(sl) if n is None else n
        if ws_bytes is None:
            ws_bytes = workspace(max(n, 1), 64, 64)
        rc = getattr(handle, entry)(fake, seq_stride, sl.ctypes.data_as(ip), fake, ref_stride, rl.ctypes.data_as(ip), n, *extra,
                                    fake, ws_bytes, fake, ops, ops_stride, n_ops, None)
        return rc, _lib.last_error()

    cases = [
        (dict(seq_lens=[3, -1], ref_lens=[3, 3]), "pair 1 has a negative length (-1, 3)"),
        (dict(seq_lens=[3, 3], ref_lens=[3, -2]), "pair 1 has a negative length (3, -2)"),
        (dict(seq_lens=[3, 65], ref_lens=[3, 3]), "pair 1: lengths (65, 3) exceed the row strides (64, 64)"),
        (dict(seq_lens=[3, 3], ref_lens=[3, 40], ref_stride=39), "pair 1: lengths (3, 40) exceed the row strides (64, 39)"),
        (dict(seq_lens=[limit + 904], ref_lens=[3], seq_stride=1 << 17), "pair 0: lengths (%d, 3) exceed the supported %d" % (limit + 904, limit)),
        (dict(seq_lens=[60, 64], ref_lens=[60, 64], ws_bytes=workspace(2, 64, 64) - 1),
         "workspace of %d bytes, %d needed (bh_%s_workspace(2, 64, 64" % (workspace(2, 64, 64) - 1, workspace(2, 64, 64), "nw" if nw else "sw")),
        (dict(seq_lens=[60, 64], ref_lens=[60, 64], ws_bytes=0), "workspace of 0 bytes"),
        (dict(seq_lens=[10, 20], ref_lens=[10, 30], ops=fake, ops_stride=48),
         "pair 1 may need %d CIGAR runs, the ops rows hold 48" % (49 if entry == "bh_sw_align" else 50)),
        (dict(seq_lens=[], ref_lens=[], n=0), "n must be positive (got 0)"),
        (dict(seq_lens=[], ref_lens=[], n=-3), "n must be positive (got -3)"),
        (dict(seq_lens=[3], ref_lens=[3], n_ops=fake), "n_ops without an ops buffer"),
        (dict(seq_lens=[3], ref_lens=[3], seq_stride=-1), "negative stride"),
    ]
    if nw:
        cases += [(dict(seq_lens=[3], ref_lens=[3], extra=(0,)), "the band half-width must be in 1..65536 (got 0)"),
                  (dict(seq_lens=[3], ref_lens=[3], extra=(65537,)), "the band half-width must be in 1..65536 (got 65537)")]
    else:
        g = default[2:]
        cases += [(dict(seq_lens=[3], ref_lens=[3], extra=(5, -4, 3, 4)), "gap_open must be in gap_extend..32767 (got open 3, extend 4)"),
                  (dict(seq_lens=[3], ref_lens=[3], extra=(5, -4, 8, 0)), "gap_extend must be at least 1 (got 0)"),
                  (dict(seq_lens=[3], ref_lens=[3], extra=(0, -4) + g), "match must be in 1..32767 (got 0)"),
                  (dict(seq_lens=[3], ref_lens=[3], extra=(5, 5) + g), "mismatch must be in -32767..match-1 (got 5)"),
                  (dict(seq_lens=[3], ref_lens=[3], extra=(5, -4, 40000, 4)), "gap_open must be in gap_extend..32767 (got open 40000, extend 4)")]
    for kwargs, text in cases:
        rc, msg = call(**kwargs)
        assert rc != 0 and msg.startswith(prefix) and text in msg, (kwargs, rc, msg)
    rc = getattr(handle, entry)(None, 64, None, fake, 64, None, 1, *default, fake, 1 << 20, fake, None, 0, None, None)
    assert rc != 0 and _lib.last_error() == prefix + "null pointer"


def test_python_surface_errors_are_raised_before_the_device_is_needed():
    from bonito_amd.align import sw_align
    # the Python surface: letters outside ACGT, unequal list lengths, too long a sequence: raised before the device is needed
    with pytest.raises(ValueError, match="outside ACGT"):
        sw_align(["ACGN"], ["ACGT"])
    with pytest.raises(ValueError, match="1 seqs against 2 refs"):
        sw_align(["ACG"], ["ACGT", "A"])
    with pytest.raises(ValueError, match="up to 4096"):
        sw_align(["A" * 4097], ["ACGT"])
    with pytest.raises(ValueError, match="padding"):
        sw_align(np.array([[1, 0, 2]], np.int8), np.array([[1, 2, 3]], np.int8))
    assert len(sw_align([], [])) == 0


def test_workspace_sizes_and_slices_equal_the_parent_commit():
    """tests/golden/align_parent.json was written by tests/golden/make_golden_align_parent.py at the commit it names, before the
    aligners' shared parts were folded: the workspace functions return the same bytes for every argument of the sweep, and the one
    slicer cuts the seeded length pairs into the slices the two former slicers made (where the local aligner's raised, the first
    pair that does not fit is the one the message named). Budgets: 1 MiB, 8 MiB, 1 GiB and one that 40 pairs fill to the byte."""
    import json
    from bonito_amd import _lib
    from bonito_amd.align import _slices
    with open(os.path.join(ROOT, "tests", "golden", "align_parent.json")) as fh:
        gold = json.load(fh)
    lib = _lib.lib()
    assert len(gold["sw_workspace"]) == 4 * 6 * 6 and len(gold["nw_workspace"]) == 4 * 7 * 7 * 4
    for n, s, r, want in gold["sw_workspace"]:
        assert lib.bh_sw_workspace(n, s, r) == want, (n, s, r)
    for n, s, r, b, want in gold["nw_workspace"]:
        assert lib.bh_nw_workspace(n, s, r, b) == want, (n, s, r, b)
    sl, rl = np.array(gold["seq_len"], np.int32), np.array(gold["ref_len"], np.int32)
    assert len(sl) == 200 and len(gold["sw_slices"]) == 8 and len(gold["nw_slices"]) == 8
    one = np.ones(len(sl), np.int64)
    for row in gold["sw_slices"]:
        pick = np.arange(len(sl)) if row["pairs"] == "all" else np.flatnonzero((sl <= 1000) & (rl <= 1000))
        order = pick[np.argsort(((sl[pick].astype(np.int64) + 511) // 512) * (rl[pick].astype(np.int64) + 63), kind="stable")]
        got, unfit = _slices(order, sl, rl, one, row["budget"], lambda k, s, r, b: lib.bh_sw_workspace(k, s, r))
        if "raises" in row:
            i = unfit[0]
            assert "one pair of lengths (%d, %d), which needs %d" % (sl[i], rl[i], lib.bh_sw_workspace(1, int(sl[i]), int(rl[i]))) \
                in row["raises"], row
        else:
            assert not unfit and [[idx.tolist(), ms, mr] for idx, ms, mr, _ in got] == row["slices"], row["budget"]
    for row in gold["nw_slices"]:
        k = row["k"]
        band = np.abs(rl.astype(np.int64) - sl) + 2 * k + 1
        size = ((sl.astype(np.int64) + 511) // 512) * np.minimum(rl.astype(np.int64), 511 + band)
        got, unfit = _slices(np.argsort(size, kind="stable"), sl, rl, band, row["budget"], lib.bh_nw_workspace)
        assert [[idx.tolist(), ms, mr, mb] for idx, ms, mr, mb in got] == row["slices"], (row["budget"], k)
        assert [int(i) for i in unfit] == row["unfit"], (row["budget"], k)

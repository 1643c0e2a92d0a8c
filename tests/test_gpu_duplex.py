"""Duplex calling on the device (-m gpu): bh_nw_align through align.nw_align and bh_sg_align through align.sg_align against the
restatements of tests/duplex_ref.py, bit for bit - every integer of the result row (except the accepted band) and the CIGAR - band
growth, the workspace budget, one long pair by its own properties, a mixed batch in any order, guard bytes around the output buffers,
duplex.call_pairs on the fixture of the reference's outputs, and `python -m bonito_amd duplex` end to end.
Every test launches each kernel once per case."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import align_ref as ar
import duplex_ref as dr
from bonito_amd import _lib, duplex
from bonito_amd import align as al
from bonito_amd.align import nw_align, sg_align, sw_align
from bonito_amd.decode import encode_sequences

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NW_LENGTHS = [1, 2, 63, 64, 65, 511, 512, 513, 1100]
SG_LENGTHS = [1, 2, 63, 64, 65, 511, 512, 513, 1000]
CONTENTS = {"random": 1, "identical": 2, "repeat": 3, "substring": 4, "planted": 5}


def mutate(rng, ref, rate):
    """A copy of `ref` with about `rate` errors per base: substitutions, insertions and deletions in equal shares."""
    out = []
    for ch in ref:
        u = rng.random()
        if u < rate / 3:
            out.append("ACGT"[(("ACGT".index(ch)) + int(rng.integers(1, 4))) % 4])
        elif u < 2 * rate / 3:
            out.append(ch)
            out.append("ACGT"[int(rng.integers(0, 4))])
        elif u >= rate:
            out.append(ch)
    return "".join(out)


def fit(rng, s, n):
    return s[:n] if len(s) >= n else s + ar.random_seq(rng, n - len(s))


def make(rng, content, m, n):
    if content == "random":
        return ar.random_seq(rng, m), ar.random_seq(rng, n)
    if content == "repeat":                                                 # one base repeated: every cell ties
        return "A" * m, "A" * n
    if content == "identical":
        s = ar.random_seq(rng, max(m, n))
        return s[:m], s[:n]
    if content == "substring":
        r = ar.random_seq(rng, max(m, n))
        lo = int(rng.integers(0, abs(n - m) + 1))
        return (r[lo:lo + m], r) if m <= n else (r, r[lo:lo + n])
    r = ar.random_seq(rng, n)                                               # errors at ~ 10 %
    return fit(rng, mutate(rng, r, 0.1), m), r


def nw_cases(content):
    rng = np.random.default_rng(CONTENTS[content])
    pairs = [make(rng, content, m, m + d) for m in NW_LENGTHS for d in (0, 1, -1, 70, -70) if m + d > 0]
    return [p[0] for p in pairs] + ["", "", "A", "ACGT"], [p[1] for p in pairs] + ["", "ACGTA", "", "G"]


def assert_nw_equals_restatement(got, seqs, refs, which=None):
    for i in (range(len(seqs)) if which is None else which):
        row, cigar = dr.nw(seqs[i], refs[i])
        have = got.table[i].tolist()
        assert have[:6] == row and have[7] == 0, (i, len(seqs[i]), len(refs[i]), have, row)
        assert got.cigar[i] == cigar, (i, len(seqs[i]), len(refs[i]))
        delta = abs(len(refs[i]) - len(seqs[i]))
        assert (row[0] - delta) // 2 <= have[6] or not (seqs[i] and refs[i])   # the acceptance inequality at the accepted band


@pytest.mark.parametrize("content", ["random", "identical", "repeat", "planted"])
def test_nw_bit_exact_against_the_restatement_crossed_lengths(content):
    seqs, refs = nw_cases(content)
    got = nw_align(seqs, refs)
    assert (got.seq_len.tolist(), got.ref_len.tolist()) == ([len(s) for s in seqs], [len(r) for r in refs])
    assert_nw_equals_restatement(got, seqs, refs)
    plain = nw_align(seqs, refs, cigar=False)                               # without the ops buffer: the same integers
    assert plain.cigar is None and (plain.table == got.table).all()


@pytest.mark.parametrize("kind", ["deletion", "insertion"])
def test_nw_band_growth_does_not_change_the_result(kind):
    """A 1500-base pair with one 300-base gap and about 5 % errors beside it: from the smallest first band (k = 1) the pair runs again
    and again until the band holds every path of its distance; from a large one it is accepted at once. The same row, the same CIGAR."""
    rng = np.random.default_rng(11)
    base = ar.random_seq(rng, 1500)
    cut = mutate(rng, base[:600], 0.05) + mutate(rng, base[900:], 0.05)
    seq, ref = (base, cut) if kind == "insertion" else (cut, base)
    row, cigar = dr.nw(seq, ref)
    assert row[3 if kind == "insertion" else 4] >= 300                      # under unit costs the gap may come out in pieces
    need = (row[0] - abs(len(ref) - len(seq))) // 2
    assert need > 8
    small, large = nw_align([seq], [ref], band=1), nw_align([seq], [ref], band=2048)
    for got in (small, large):
        assert got.table[0, :6].tolist() == row and got.status[0] == 0 and got.cigar[0] == cigar
        assert need <= got.band[0]                                          # the acceptance inequality
    assert need <= small.band[0] < 2 * max(need, 1) and large.band[0] == 2048   # doubled from 1: the first power of two that holds


def test_nw_pair_that_does_not_fit_the_budget_is_flagged():
    rng = np.random.default_rng(12)
    r = ar.random_seq(rng, 3000)
    seqs, refs = [mutate(rng, r, 0.05), "ACGT", ar.random_seq(rng, 3000)], [r, "ACGA", r]
    got = nw_align(seqs, refs, workspace_budget=1 << 20)
    assert got.status.tolist() == [0, 0, al.NW_NO_FIT] and got.cigar[2] == "" and got.num_runs[2] == 0
    assert got.distance[2] >= dr.edit_distance(seqs[2], refs[2])             # the last banded distance: an upper bound
    assert got.distance[0] == dr.edit_distance(seqs[0], refs[0]) and got.cigar[1] == "3=1X"
    with pytest.raises(ValueError, match="65536"):
        nw_align(["A" * 65537], ["A"])


def test_nw_long_pair_by_its_own_properties():
    """About 20 000 bases at about 5 %, lengths differing by a few hundred: 40 passes, a band of over a thousand diagonals, more
    than 2^32 cells in the full matrix."""
    rng = np.random.default_rng(13)
    ref = ar.random_seq(rng, 20000)
    seq = mutate(rng, ref[:19700], 0.05)
    got = nw_align([seq], [ref])
    assert got.status[0] == 0 and got.distance[0] == dr.edit_distance(seq, ref)
    assert got.distance[0] > 1000 and abs(len(ref) - len(seq)) > 200
    i = j = 0
    cnt = {c: 0 for c in "=XID"}
    a, b = np.frombuffer(seq.encode(), np.uint8), np.frombuffer(ref.encode(), np.uint8)
    runs = ar.parse(got.cigar[0])
    assert all(x[1] != y[1] for x, y in zip(runs, runs[1:])) and len(runs) == got.num_runs[0]
    for k, op in runs:
        cnt[op] += k
        if op in "=X":
            assert ((a[i:i + k] == b[j:j + k]) == (op == "=")).all()
            i, j = i + k, j + k
        elif op == "I":
            i += k
        else:
            j += k
    assert (i, j) == (len(seq), len(ref))
    assert cnt["X"] + cnt["I"] + cnt["D"] == got.distance[0]
    assert [cnt[c] for c in "=XID"] == got.table[0, 1:5].tolist()


def test_nw_mixed_batch_in_any_order_under_a_small_budget():
    rng = np.random.default_rng(14)
    seqs, refs = [], []
    for k in range(256):
        n = int(rng.choice([0, 1, 5, 40, 200, 511, 513, 700, 1300]) + rng.integers(0, 30)) if k % 16 else 0
        r = ar.random_seq(rng, n)
        s = "" if k % 37 == 0 else mutate(rng, r, float(rng.choice([0.02, 0.1])))
        if k % 11 == 0:
            s = ar.random_seq(rng, int(rng.integers(0, 600)))               # nothing in common: the band grows
        seqs.append(s); refs.append(r)
    perm = rng.permutation(256)
    base = nw_align(seqs, refs)
    shuffled = nw_align([seqs[i] for i in perm], [refs[i] for i in perm], workspace_budget=2 << 20)
    assert (shuffled.table == base.table[perm]).all() and shuffled.cigar == [base.cigar[i] for i in perm]
    assert (base.status == 0).all() and len(set(base.band.tolist())) > 1
    sample = sorted(rng.choice(256, size=16, replace=False).tolist())
    assert_nw_equals_restatement(base, seqs, refs, which=sample)
    single = nw_align([seqs[i] for i in sample[:6]], [refs[i] for i in sample[:6]], band=8)
    assert (single.table[:, :6] == base.table[sample[:6], :6]).all() and single.cigar == [base.cigar[i] for i in sample[:6]]
    codes = nw_align(*[torch.from_numpy(np.array([[("ACGT".index(c) + 1) for c in s] + [0] * (1400 - len(s)) for s in x], np.int8))
                       for x in (seqs, refs)], cigar=False)
    assert (codes.table == base.table).all()                                # code planes in, the same results


def sg_cases(content):
    rng = np.random.default_rng(20 + CONTENTS[content])
    pairs = [make(rng, content, m, n) for m in SG_LENGTHS for n in SG_LENGTHS]
    return [p[0] for p in pairs] + ["", "", "ACG"], [p[1] for p in pairs] + ["", "AC", ""]


@pytest.mark.parametrize("content", ["random", "substring", "repeat", "planted"])
def test_sg_bit_exact_against_the_restatement_crossed_lengths(content):
    seqs, refs = sg_cases(content)
    before = sw_align(seqs, refs, cigar=True)
    got = sg_align(seqs, refs)
    after = sw_align(seqs, refs, cigar=True)
    assert (before.table == after.table).all() and before.cigar == after.cigar     # the local mode beside it is untouched
    for i, (s, r) in enumerate(zip(seqs, refs)):
        row, cigar = dr.sg(s, r, *dr.SG_DEFAULT)
        assert got.table[i].tolist() == row, (i, len(s), len(r), got.table[i].tolist(), row)
        assert got.cigar[i] == cigar, (i, len(s), len(r))
        assert dr.lengths(ar.parse(got.cigar[i])) == (len(s), len(r))               # the CIGAR spans both sequences
    if content == "substring":
        whole = [i for i, (s, r) in enumerate(zip(seqs, refs)) if s and r and len(s) <= len(r)]
        assert all(got.num_correct[i] == len(seqs[i]) and got.num_mismatches[i] == 0 for i in whole)
    other = sg_align(seqs[:20], refs[:20], 2, -3, 5, 2)                             # other parameters
    for i in range(20):
        assert (other.table[i].tolist(), other.cigar[i]) == dr.sg(seqs[i], refs[i], 2, -3, 5, 2)


def test_guard_bytes_around_the_output_buffers():
    """The result, ops and run-count buffers sit inside larger allocations filled with a pattern: the kernels write their own
    elements and nothing on either side."""
    rng = np.random.default_rng(15)
    refs = [ar.random_seq(rng, n) for n in (1, 64, 513, 700, 0, 300)]
    seqs = [mutate(rng, r, 0.1) for r in refs[:4]] + ["ACGT", ""]
    sc, sl = encode_sequences(seqs)
    rc, rl = encode_sequences(refs)
    sl, rl = sl.numpy().astype(np.int32), rl.numpy().astype(np.int32)
    n, lib, ip = len(seqs), _lib.lib(), C.POINTER(C.c_int32)
    s_dev, r_dev = sc.contiguous().cuda(), rc.contiguous().cuda()
    stride, pad, fill = int((sl + rl).max()), 64, 0x5A5A5A5A
    for name, width in (("nw", 8), ("sg", 10), ("sw", 10)):
        res = torch.full((n * width + 2 * pad,), fill, dtype=torch.int32, device="cuda")
        ops = torch.full((n * stride + 2 * pad,), fill, dtype=torch.int32, device="cuda")
        cnt = torch.full((n + 2 * pad,), fill, dtype=torch.int32, device="cuda")
        ptrs = [_lib.ptr(t[pad:]) for t in (res, ops, cnt)]
        if name == "nw":
            band = int(np.abs(rl - sl).max()) + 2 * 512 + 1
            nbytes = lib.bh_nw_workspace(n, int(sl.max()), int(rl.max()), band)
            ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            _lib.check(lib.bh_nw_align(_lib.ptr(s_dev), s_dev.shape[1], sl.ctypes.data_as(ip), _lib.ptr(r_dev), r_dev.shape[1],
                                       rl.ctypes.data_as(ip), n, 512, _lib.ptr(ws), nbytes, ptrs[0], ptrs[1], stride, ptrs[2],
                                       _lib.stream_ptr(s_dev.device)), "bh_nw_align")
            want = [dr.nw(s, r) for s, r in zip(seqs, refs)]
        else:                                                                 # the semi-global and the local mode of one kernel pair
            entry, scoring = (lib.bh_sg_align, dr.SG_DEFAULT) if name == "sg" else (lib.bh_sw_align, (5, -4, 8, 4))
            nbytes = lib.bh_sw_workspace(n, int(sl.max()), int(rl.max()))
            ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            _lib.check(entry(_lib.ptr(s_dev), s_dev.shape[1], sl.ctypes.data_as(ip), _lib.ptr(r_dev), r_dev.shape[1],
                             rl.ctypes.data_as(ip), n, *scoring, _lib.ptr(ws), nbytes, ptrs[0], ptrs[1], stride, ptrs[2],
                             _lib.stream_ptr(s_dev.device)), "bh_%s_align" % name)
            want = [(dr.sg if name == "sg" else ar.sw)(s, r, *scoring) for s, r in zip(seqs, refs)]
        torch.cuda.synchronize()
        res, ops, cnt = res.cpu().numpy(), ops.cpu().numpy(), cnt.cpu().numpy()
        for t in (res, ops, cnt):
            assert (t[:pad] == fill).all() and (t[-pad:] == fill).all(), name
        rows = res[pad:-pad].reshape(n, width)
        runs = ops[pad:-pad].reshape(n, stride)
        for i in range(n):
            k = len(ar.parse(want[i][1]))
            assert rows[i, :len(want[i][0])].tolist() == want[i][0] and cnt[pad + i] == k, (name, i)
            assert al.runs_to_cigar(runs[i, :k].view(np.uint32)) == want[i][1], (name, i)
            assert (runs[i, k:] == fill).all(), (name, i)                     # nothing beyond a pair's own runs


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "duplex_cases.json")) as fh:
        return json.load(fh)["cases"]


def test_call_pairs_equals_the_fixture(golden):
    stats = {}
    got = duplex.call_pairs([c["temp_seq"] for c in golden], [c["temp_qstring"] for c in golden], [c["comp_seq"] for c in golden],
                            [c["comp_qstring"] for c in golden], stats=stats)
    for c, g in zip(golden, got):
        assert g == (c["sequence"], c["qstring"]), c["name"]
    assert stats == {"unaligned": 0, "kept_nw": 0}
    aligned = duplex.adj_align([c["temp_seq"] for c in golden], [dr.revcomp(c["comp_seq"]) for c in golden])
    assert aligned == [ar.parse(c["cigar"]) for c in golden]


def test_duplex_command_line_end_to_end(tmp_path, golden):
    from bonito_amd.util import mean_qscore_from_qstring
    cases = [c for c in golden if c["name"].startswith("random_")][:6] + [c for c in golden if c["name"] == "no_long_match"]
    assert len(cases) == 7
    with open(tmp_path / "calls.fastq", "w") as fh:
        for k, c in enumerate(cases):
            fh.write("@t%d qs:f:10.0\n%s\n+\n%s\n@c%d\n%s\n+\n%s\n" % (k, c["temp_seq"], c["temp_qstring"], k, c["comp_seq"],
                                                                    c["comp_qstring"]))
    pairs = [("t%d" % k, "c%d" % k) for k in range(7)] + [("t0", "nowhere")]      # 8 pairs: one junk pair (6), one missing id
    (tmp_path / "pairs.txt").write_text("template complement\n" + "".join("%s %s\n" % p for p in pairs))
    run = subprocess.run([sys.executable, "-m", "bonito_amd", "duplex", str(tmp_path / "calls.fastq"), str(tmp_path / "pairs.txt"),
                          "--batch", "5"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert run.returncode == 0, run.stderr
    want = duplex.call_pairs([c["temp_seq"] for c in cases], [c["temp_qstring"] for c in cases], [c["comp_seq"] for c in cases],
                             [c["comp_qstring"] for c in cases])
    assert want == [(c["sequence"], c["qstring"]) for c in cases] and want[6] == ("", "")
    lines = run.stdout.split("\n")
    assert lines[-1] == "" and len(lines) == 4 * 6 + 1
    for k in range(6):
        head, seq, plus, qual = lines[4 * k:4 * k + 4]
        assert head == "@t%d;c%d qs:i:%d" % (k, k, round(mean_qscore_from_qstring(want[k][1])))
        assert (seq, plus, qual) == (want[k][0], "+", want[k][1])
    err = run.stderr
    assert "> completed reads: 8\n" in err and "> pairs with a missing read: 1\n" in err and "> empty calls: 2\n" in err
    assert "> duration: " in err and "> bases per second " in err

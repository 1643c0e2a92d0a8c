"""Smith-Waterman alignment on the device (-m gpu): bh_sw_align through align.sw_align against the restatement (tests/align_ref.py),
bit for bit - all ten integers and the CIGAR, exact integer equality - plus checks that do not depend on the restatement, planted
edits, a mixed batch of 512 pairs in any order and under any workspace budget, and `python -m bonito_amd evaluate` end to end.
Every test runs the kernel once per case."""
import re

import numpy as np
import pytest
import torch

import align_ref as ar
from bonito_amd.align import sw_align

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 63, 64, 65, 511, 512, 513, 1000]


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
    """`s` cut or padded with random bases to exactly n bases"""
    return s[:n] if len(s) >= n else s + ar.random_seq(rng, n - len(s))


def crossed(content):
    rng = np.random.default_rng({"random": 1, "identical": 2, "repeat": 3, "substring": 4, "planted": 5}[content])
    seqs, refs = [], []
    for m in LENGTHS:
        for n in LENGTHS:
            if content == "random":
                seqs.append(ar.random_seq(rng, m)); refs.append(ar.random_seq(rng, n))
            elif content == "repeat":                                       # one base repeated: every cell ties
                seqs.append("A" * m); refs.append("A" * n)
            elif content == "identical":
                if m == n:
                    s = ar.random_seq(rng, m)
                    seqs.append(s); refs.append(s)
            elif content == "substring":
                if m <= n:
                    r = ar.random_seq(rng, n)
                    lo = int(rng.integers(0, n - m + 1))
                    seqs.append(r[lo:lo + m]); refs.append(r)
            else:                                                           # errors at ~ 10 %, both lengths as crossed
                r = ar.random_seq(rng, n)
                seqs.append(fit(rng, mutate(rng, r, 0.1), m)); refs.append(r)
    return seqs, refs


def assert_equals_restatement(got, seqs, refs, scoring=ar.DEFAULT, which=None):
    for i in (range(len(seqs)) if which is None else which):
        row, cigar = ar.sw(seqs[i], refs[i], *scoring)
        assert got.table[i].tolist() == row, (i, len(seqs[i]), len(refs[i]), got.table[i].tolist(), row)
        assert got.cigar[i] == cigar, (i, len(seqs[i]), len(refs[i]))


@pytest.mark.parametrize("content", ["random", "identical", "repeat", "substring", "planted"])
def test_bit_exact_against_the_restatement_crossed_lengths(content):
    seqs, refs = crossed(content)
    got = sw_align(seqs, refs, cigar=True)
    assert (got.seq_len.tolist(), got.ref_len.tolist()) == ([len(s) for s in seqs], [len(r) for r in refs])
    assert_equals_restatement(got, seqs, refs)
    plain = sw_align(seqs, refs)                                            # without the ops buffer: the same ten integers
    assert plain.cigar is None and (plain.table == got.table).all()


def test_bit_exact_against_the_restatement_4096():
    """One 4096 x 4096 pair (eight passes, 8 MiB of traceback bits, errors at ~ 10 % so that the path crosses every pass) and the two
    thin shapes. The restatement of the large pair is what this test costs: about 3 s of numpy."""
    rng = np.random.default_rng(6)
    r = ar.random_seq(rng, 4096)
    seqs = [fit(rng, mutate(rng, r, 0.1), 4096), ar.random_seq(rng, 4096), r[1000:1037]]
    refs = [r, r[2000:2037], r]
    got = sw_align(seqs, refs, cigar=True)
    assert_equals_restatement(got, seqs, refs)
    assert got.num_correct[0] > 3000 and got.align_seq_end[0] > 3584        # the path does end in the last pass


def test_checks_that_do_not_depend_on_the_restatement():
    rng = np.random.default_rng(7)
    seqs, refs = [], []
    for k in range(96):
        n = int(rng.integers(1, 1300))
        r = ar.random_seq(rng, n)
        s = mutate(rng, r, float(rng.choice([0.02, 0.1, 0.3])))
        if k % 4 == 0:
            lo = int(rng.integers(0, len(s) + 1))
            s = ar.random_seq(rng, int(rng.integers(0, 80))) + s[lo:]           # clipped on the left
        if k % 5 == 0:
            s = s + ar.random_seq(rng, int(rng.integers(0, 80)))
        seqs.append(s); refs.append(r)
    for scoring in (ar.DEFAULT, (2, -3, 5, 2)):
        got = sw_align(seqs, refs, *scoring, cigar=True)
        swapped = sw_align(refs, seqs, *scoring)
        mirrored = sw_align([s[::-1] for s in seqs], [r[::-1] for r in refs], *scoring)
        for i, (s, r) in enumerate(zip(seqs, refs)):
            a = got[i]
            if a.score == 0:
                assert got.table[i].tolist() == ar.EMPTY and a.cigar == ""
                continue
            # replaying the ops consumes exactly the reported spans; '=' on equal bases, 'X' on unequal ones (asserted in replay);
            # rescoring the ops with the four parameters gives the score
            score, seq_end, ref_end, cnt = ar.replay(a.cigar, s, r, a.align_seq_start, a.align_ref_start, *scoring)
            assert (score, seq_end, ref_end) == (a.score, a.align_seq_end, a.align_ref_end), i
            assert [cnt[c] for c in "=XID"] == [a.num_correct, a.num_mismatches, a.num_insertions, a.num_deletions]
            assert 0 <= a.align_seq_start <= a.align_seq_end < len(s) and 0 <= a.align_ref_start <= a.align_ref_end < len(r)
            ops = ar.parse(a.cigar)
            assert ops[0][1] in "=X" and ops[-1][1] == "=" and len(ops) == got.num_runs[i]
            assert all(x[1] != y[1] for x, y in zip(ops, ops[1:]))                # run-length: neighbours differ
        # only the score: the tie-breaks are not symmetric, so the paths may differ
        assert (swapped.score == got.score).all() and (mirrored.score == got.score).all()


def test_planted_edits_on_the_device():
    rng = np.random.default_rng(8)
    seqs, refs, want = [], [], []
    for k in range(64):
        length = int(rng.integers(150, 401))
        total = int(rng.integers(1, min((length - 41) // 25 + 1, 9) + 1))
        cut = np.sort(rng.integers(0, total + 1, size=2))
        counts = [int(cut[0]), int(cut[1] - cut[0]), int(total - cut[1])]
        s, r = ar.planted(rng, length, *counts)
        seqs.append(s); refs.append(r); want.append([length - counts[0] - counts[2]] + counts)
    got = sw_align(seqs, refs)
    assert got.table[:, 1:5].tolist() == want
    assert (got.align_ref_start == 0).all() and (got.align_ref_end == got.ref_len - 1).all()
    assert (got.align_seq_start == 0).all() and (got.align_seq_end == got.seq_len - 1).all()


def test_batch_of_512_in_any_order_under_any_budget():
    rng = np.random.default_rng(9)
    seqs, refs = [], []
    for k in range(512):
        n = int(rng.choice([0, 1, 5, 40, 200, 511, 513, 700, 900]) + rng.integers(0, 30)) if k % 16 else 0
        r = ar.random_seq(rng, n)
        s = "" if k % 37 == 0 else mutate(rng, r, 0.1)
        if k % 11 == 0:
            s = ar.random_seq(rng, int(rng.integers(0, 600)))                   # nothing in common
        seqs.append(s); refs.append(r)
    assert sum(1 for s in seqs if not s) > 10 and sum(1 for r in refs if not r) > 10
    perm = rng.permutation(512)
    sample = sorted(rng.choice(512, size=24, replace=False).tolist())
    for scoring in (ar.DEFAULT, (2, -3, 5, 2)):
        base = sw_align(seqs, refs, *scoring, cigar=True)
        shuffled = sw_align([seqs[i] for i in perm], [refs[i] for i in perm], *scoring, cigar=True)
        assert (shuffled.table == base.table[perm]).all() and shuffled.cigar == [base.cigar[i] for i in perm]
        sliced = sw_align(seqs, refs, *scoring, cigar=True, workspace_budget=4 << 20)     # a few pairs of 900 per launch
        assert (sliced.table == base.table).all() and sliced.cigar == base.cigar
        assert_equals_restatement(base, seqs, refs, scoring, which=sample)
        empty = [i for i in range(512) if not seqs[i] or not refs[i]]
        assert all(base.table[i].tolist() == ar.EMPTY and base.cigar[i] == "" for i in empty)
    codes = sw_align(*[torch.from_numpy(np.array([[("ACGT".index(c) + 1) for c in s] + [0] * (1200 - len(s)) for s in x], np.int8))
                       for x in (seqs, refs)])
    assert (codes.table == sw_align(seqs, refs).table).all()                    # code planes in, the same results
    with pytest.raises(ValueError, match="cannot hold one pair"):
        sw_align(seqs, refs, workspace_budget=1 << 16)


def test_evaluate_cli_prints_accuracy_and_writes_the_alignments(tmp_path, capsys):
    import json
    from conftest import load_nn_fixture
    from bonito_amd.cli import evaluate
    cfg, sd, _, _ = load_nn_fixture("lstm64_sl3")

    def tv(v):
        if isinstance(v, bool):
            return "true" if v else "false"
        if isinstance(v, str):
            return json.dumps(v)
        if isinstance(v, list):
            return "[" + ", ".join(tv(i) for i in v) + "]"
        return repr(v)

    mdir, ddir, odir = tmp_path / "model", tmp_path / "chunks", tmp_path / "out"
    mdir.mkdir(); ddir.mkdir()
    lines = ['[model]', 'package = "bonito.crf"', '[labels]', 'labels = ["N", "A", "C", "G", "T"]', '[input]',
             'features = 1', '[global_norm]', 'state_len = 3', '[basecaller]', 'batchsize = 8', 'chunksize = 1200',
             'overlap = 120', '[encoder]', 'type = "serial"']
    for sub in cfg["sublayers"]:
        lines.append("[[encoder.sublayers]]")
        lines += ["%s = %s" % (k, tv(v)) for k, v in sub.items()]
    (mdir / "config.toml").write_text("\n".join(lines) + "\n")
    sd = {k: (v * 30.0 if k.endswith("linear.weight") else v) for k, v in sd.items()}
    torch.save(sd, str(mdir / "weights_1.tar"))
    rng = np.random.default_rng(10)
    n = 12
    np.save(ddir / "chunks.npy", rng.standard_normal((n, 1200)).astype(np.float32))
    lens = rng.integers(40, 161, size=n).astype(np.uint16)
    refs = rng.integers(1, 5, size=(n, 160)).astype(np.uint8)
    for i in range(n):
        refs[i, lens[i]:] = 0
    np.save(ddir / "references.npy", refs)
    np.save(ddir / "reference_lengths.npy", lens)
    args = evaluate.argparser().parse_args([str(mdir), "--directory", str(ddir), "--weights", "1", "--chunks", str(n),
                                            "--batchsize", "8", "--output_dir", str(odir)])
    assert evaluate.main(args) == 0
    out = capsys.readouterr().out
    acc = re.search(r"^\* accuracy\s+([0-9.]+)%$", out, flags=re.M)
    assert acc and 0.0 <= float(acc.group(1)) <= 100.0
    assert "* loss mean" in out and "* loss median" in out and "* sub-rate" in out and "not computed" not in out

    def fasta(path):
        rows = path.read_text().split("\n")
        return rows[1::2][:n]

    called, known = fasta(odir / "seqs.fasta"), fasta(odir / "refs.fasta")
    assert len(called) == n and known == ["".join("NACGT"[c] for c in refs[i, :lens[i]]) for i in range(n)]
    summ = (odir / "summ.txt").read_text().split("\n")
    assert summ[0].split("\t")[1:3] == ["loss", "accuracy"] and len(summ) == n + 2
    for i in range(n):
        row, _ = ar.sw(called[i], known[i])
        total = sum(row[1:5])
        f = summ[1 + i].split("\t")
        assert int(f[0]) == i and float(f[2]) == pytest.approx(row[1] / total if total else 0.0, abs=1e-6)
        assert [int(x) for x in f[3:]] == row[1:5] + [len(known[i]), len(called[i])] + row[5:9]

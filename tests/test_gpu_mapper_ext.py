"""The end extension on the device (csrc/mapper.hip ``bh_map_extend``, ``Aligner.map_batch(extend_ends=True)``) against its definition
tests/mapper_ext_ref.py: every comparison is on integers or strings and exact."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import mapper_cases as cases
import mapper_ext_ref as X
import mapper_ref as M

pytestmark = pytest.mark.gpu

CAP = 2 * X.EXT_MAX + X.EXT_BAND
GUARD = 0x5A5A5A5A


def _aligner(contigs, **kw):
    from bonito_amd.aligner import Aligner
    return Aligner(list(contigs), **kw)


def _end_cases():
    """-> (contigs [(name, seq)], reads [str as given], ends [(read, strand, side, q position, contig, r position)]): the query tail
    `qt` and the reference tail `rt` (nearest base first) of every case are planted behind (side 1) or, reversed, in front of
    (side 0) a stretch that stands in for the span, on either strand."""
    rng = random.Random(23)
    contigs, reads, ends = [], [], []

    def add(qt, rt, side, strand, q_span=20, r_span=10):
        qs, rs = cases.random_seq(rng, q_span), cases.random_seq(rng, r_span)
        aligned = qs + qt if side else qt[::-1] + qs
        contig = rs + rt if side else rt[::-1] + rs
        reads.append(M.revcomp(aligned) if strand else aligned)
        contigs.append(("c%d" % len(contigs), contig))
        ends.append((len(reads) - 1, strand, side, q_span if side else len(qt), len(contigs) - 1, r_span if side else len(rt)))

    combos = [(side, strand) for side in (0, 1) for strand in (0, 1)]
    for n in (0, 1, 31, 32, 33, 63, 64, 65, 127, 511, 512, 600):           # 600 is capped at EXT_MAX
        for rate in (0.0, 0.06):
            qt = cases.random_seq(rng, n)
            for side, strand in (combos if n < 500 else combos[(n + (rate > 0)) % 2::2]):
                add(qt, cases.mutate(rng, qt, rate) + cases.random_seq(rng, 40), side, strand)
    for _ in range(12):                                                   # more tails at 6 % with indels, odd lengths
        for side, strand in combos:
            qt = cases.random_seq(rng, rng.randint(40, 150))
            add(qt, cases.mutate(rng, qt, 0.06) + cases.random_seq(rng, 40), side, strand)
    qt = cases.random_seq(rng, 64)
    for cut in (0, 1, 40):                                                # the contig ends 0, 1, 40 bases beyond the span
        for side, strand in combos:
            add(qt, qt[:cut], side, strand)
    unit = "".join(rng.choice("ACT") for _ in range(100))
    for gap in (32, 33):                                                  # a gap of the band's width is bridged, one more is not
        for side, strand in ((0, 0), (1, 1), (1, 0), (0, 1)):
            add(unit, "G" * gap + unit, side, strand)                     # D
            add("G" * gap + unit, unit, side, strand)                     # I
    for qt, rt in (("TAC", "GAC"), ("TACG", "GACG"), ("ACGTAC", "ACGAAC"), ("AAAA", "CCCC"), ("AACCC", "ACCC"), ("ACNGT", "ACNGT"),
                   ("ACGTNACGTA", "ACGTCACGTA"), ("ACGTCACGTA", "ACGTNACGTA"), ("NNNN", "NNNN")):
        for side, strand in ((0, 0), (1, 1), (1, 0)):
            add(qt, rt, side, strand)
    add("ACGTACGTAC", "ACGTACGTAC", 1, 0, q_span=0, r_span=0)             # a span of no bases at the start of read and contig
    return contigs, reads, ends


def _call(al, reads, ends_global, guard_rows=1):
    """-> (rc, result [n, 4], runs [n, CAP], the guard rows around both)"""
    from bonito_amd import _lib
    from bonito_amd.aligner import encode
    codes = [encode(s) for s in reads]
    lens = np.array([len(c) for c in codes], np.int32)
    plane = np.zeros((len(reads), max(1, int(lens.max()))), np.int8)
    for i, c in enumerate(codes):
        plane[i, :len(c)] = c
    dev_plane, dev_lens = torch.from_numpy(plane).cuda(), torch.from_numpy(lens).cuda()
    n = len(ends_global)
    dev_ends = torch.tensor(np.asarray(ends_global, np.int32).reshape(-1, 6), device="cuda")
    result = torch.full((n + 2, 4), GUARD, dtype=torch.int32, device="cuda")
    runs = torch.full((n + 2, CAP), GUARD, dtype=torch.int32, device="cuda")
    rc = _lib.lib().bh_map_extend(_lib.ptr(dev_plane), plane.shape[1], _lib.ptr(dev_lens), len(reads), _lib.ptr(al._ref), int(al._ref.numel()),
                                  _lib.ptr(dev_ends) if n else None, n, _lib.ptr(result[1:]), _lib.ptr(runs[1:]), CAP, None)
    torch.cuda.synchronize()
    return rc, result.cpu().numpy(), runs.cpu().numpy()


def test_extend_kernel_equals_the_restatement():
    contigs, reads, ends = _end_cases()
    assert 180 <= len(ends) <= 260
    al = _aligner(contigs)
    starts = al._starts
    # the first contig's left end sits at position 0 of the concatenated reference, the last contig's right end at its last base
    ends = ends + [(0, 0, 0, 5, 0, 0), (len(reads) - 1, 0, 1, 3, len(contigs) - 1, len(contigs[-1][1]))]
    rows = [(rd, st, side, qp, int(starts[ci]) + rp, int(starts[ci]) + (len(contigs[ci][1]) if side else 0)) for rd, st, side, qp, ci, rp in ends]
    assert rows[-2][4] == 0 and rows[-1][4] == int(al._ref.numel())
    rc, result, runs = _call(al, reads, rows)
    assert rc == 0
    assert (result[0] == GUARD).all() and (result[-1] == GUARD).all() and (runs[0] == GUARD).all() and (runs[-1] == GUARD).all()
    taken = longest = 0
    for e, (rd, st, side, qp, ci, rp) in enumerate(ends):
        q = M.codes(M.revcomp(reads[rd]) if st else reads[rd])
        score, i, j, words = X.extend_end(q, M.codes(contigs[ci][1]), qp, rp, side)
        assert result[e + 1].tolist() == [score, i, j, len(words)], (e, ends[e])
        assert runs[e + 1, :len(words)].view(np.uint32).tolist() == words, (e, ends[e])
        assert (runs[e + 1, len(words):] == GUARD).all(), e                # nothing is written behind the runs
        taken += score > 0
        longest = max(longest, i)
    assert taken > 120 and longest == X.EXT_MAX


def test_extend_argument_checks_and_empty_call():
    from bonito_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(4096)                                                 # never read: every case is refused in front of any device call

    def call(reads=p, lens=p, ref=p, ends=p, result=p, runs=p, n_ends=4, cap=CAP, n_reads=2, stride=100, ref_len=1000):
        return lib.bh_map_extend(reads, stride, lens, n_reads, ref, ref_len, ends, n_ends, result, runs, cap, None), _lib.last_error()
    for name in ("reads", "lens", "ref", "ends", "result", "runs"):
        rc, msg = call(**{name: None})
        assert rc != 0 and "null pointer" in msg, name
    rc, msg = call(n_ends=-1)
    assert rc != 0 and "n_ends must not be negative" in msg
    rc, msg = call(cap=CAP - 1)
    assert rc != 0 and "runs_cap must be at least %d" % CAP in msg
    rc, msg = call(stride=-1)
    assert rc != 0 and "negative" in msg
    assert call(n_ends=0)[0] == 0 and call(n_ends=0, reads=None, ends=None, result=None, runs=None)[0] == 0
    assert lib.bh_map_extend_max() == X.EXT_MAX and lib.bh_map_extend_band() == X.EXT_BAND
    # on the device: no end, nothing written
    contigs = [("c", "ACGT" * 30)]
    al = _aligner(contigs)
    rc, result, runs = _call(al, ["ACGT" * 5], [])
    assert rc == 0 and (result == GUARD).all() and (runs == GUARD).all()
    # an end that does not fit its read, its contig limit or the reference is flagged and not read
    bad = [(0, 0, 1, 21, 10, 120), (1, 0, 1, 5, 10, 120), (0, 2, 1, 5, 10, 120), (0, 0, 1, 5, 121, 121), (0, 0, 1, 5, 50, 40), (0, 0, 0, 5, 50, 60),
           (0, 0, 1, -1, 10, 120), (0, 0, 1, 20, 120, 120)]
    rc, result, runs = _call(al, ["ACGT" * 5], bad)
    assert rc == 0 and result[1:-1].tolist() == [[0, 0, 0, -1]] * 7 + [[0, 0, 0, 0]] and (runs == GUARD).all()
    with pytest.raises(RuntimeError, match="does not fit"):
        al.extend(torch.zeros((1, 20), dtype=torch.int8, device="cuda"), torch.tensor([20], dtype=torch.int32, device="cuda"),
                  np.array([bad[0]], np.int32))


@pytest.fixture(scope="module")
def planted_extended():
    contigs, reads = cases.planted()
    index = M.Index(contigs)
    return [X.map_read(r[0], index) for r in reads]


def test_map_batch_with_extended_ends_equals_the_restatement(planted_extended):
    contigs, reads = cases.planted()
    al = _aligner(contigs)
    seqs = [r[0] for r in reads]
    got = al.map_batch(seqs + ["ACGTACGT", ""], extend_ends=True)
    assert got[-2:] == [None, None] and al.timings["extend"] > 0
    names = dict(contigs)
    for g, want, seq in zip(got, planted_extended, seqs):
        assert (g is None) == (want is None)
        if want is not None:
            assert g.as_dict() == want
            cases.check_replay(g, seq, names[g.ctg])
    # the option off: nothing moved
    plain = al.map_batch(seqs)
    for g, want in zip(plain, cases.planted_expected()):
        assert (g is None) == (want is None) and (want is None or g.as_dict() == want)
    assert any(g.as_dict() != p.as_dict() for g, p in zip(got, plain) if g is not None)
    # the constructor's value is the default of the call
    on = _aligner(contigs, extend_ends=True)
    assert [m and m.as_dict() for m in on.map_batch(seqs[:8])] == planted_extended[:8]
    assert [m and m.as_dict() for m in on.map_batch(seqs[:8], extend_ends=False)] == cases.planted_expected()[:8]


def test_a_substitution_near_the_end_is_crossed_only_with_the_option():
    rng = random.Random(9)
    contig = cases.random_seq(rng, 4000)
    read = contig[1000:1600]
    read = read[:-6] + ("A" if read[-6] != "A" else "C") + read[-5:]
    al = _aligner([("c", contig)])
    index = M.Index([("c", contig)])
    for seq in (read, M.revcomp(read)):
        old, new = al.map_batch([seq])[0], al.map_batch([seq], extend_ends=True)[0]
        assert old.as_dict() == M.map_read(seq, index) and new.as_dict() == X.map_read(seq, index)
        assert (new.q_st, new.q_en) == (0, len(seq)) and (new.r_st, new.r_en) == (1000, 1600) and new.NM == 1
        assert old.q_en - old.q_st == len(seq) - 6 and old.NM == 0
        cases.check_replay(new, seq, contig)

"""The mapper's definition (tests/mapper_ref.py) against independent evaluations of its own rules, and the host glue of
bonito_amd/aligner.py, bonito_amd/io.py and the basecaller's parser. No GPU."""
import gzip
import itertools
import json
import os
import random
import types

import numpy as np
import pytest

import duplex_ref
import mapper_cases as cases
import mapper_ref as M
from conftest import GOLDEN


# ---- sketch ----------------------------------------------------------------------------------------------------------------------

def naive_sketch(seq, k, w):
    """The definition read literally, O(L w): every window on its own."""
    mask = (1 << (2 * k)) - 1
    L = len(seq)
    keys = {}
    for p in range(k - 1, L):
        kmer = seq[p - k + 1:p + 1]
        if any(c not in "ACGT" for c in kmer):
            continue
        fw = rv = 0
        for t, c in enumerate(kmer):
            fw |= "ACGT".index(c) << (2 * (k - 1 - t))
            rv |= (3 - "ACGT".index(c)) << (2 * t)
        kf, kr = M.mix(fw, mask), M.mix(rv, mask)
        if kf != kr:
            keys[p] = (min(kf, kr), int(kr < kf))
    chosen = set()
    if L >= k:
        for e in range(min(k + w - 2, L - 1), L):
            best = None
            for p in range(max(k - 1, e - w + 1), e + 1):
                if p in keys and (best is None or keys[p][0] < keys[best][0]):
                    best = p
            if best is not None:
                chosen.add(best)
    return [(keys[p][0], p, keys[p][1]) for p in sorted(chosen)]


def test_mix_is_invertible_on_small_words():
    for bits in (8, 11):
        mask = (1 << bits) - 1
        assert sorted(M.mix(x, mask) for x in range(mask + 1)) == list(range(mask + 1))


@pytest.mark.parametrize("k,w", [(15, 10), (11, 1), (28, 64), (11, 64), (28, 1), (12, 5)])
def test_sketch_equals_the_naive_evaluation(k, w):
    rng = random.Random(1000 * k + w)
    tile = 512
    lengths = [0, k - 1, k, k + w - 2, k + w - 1, k + w, 200, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1]
    unit = cases.random_seq(rng, 37)
    r = cases.random_seq(rng, 900)
    seqs = [cases.random_seq(rng, n) for n in lengths] + [
        "A" * 300, unit * 12, "ACGT" * 100, "AT" * 150, r[:300] + "N" * 5 + r[300:600] + "N" * 40 + r[600:] + "N", "N" * 100]
    for s in seqs:
        assert M.sketch(s, k, w) == naive_sketch(s, k, w), (len(s), s[:16])
    if k % 2 == 0:
        assert M.sketch("AT" * 150, k, w) == []                          # every k-mer is its own reverse complement
    assert len(M.sketch("A" * 300, k, w)) == 300 - k - min(w, 300 - k + 1) + 2        # equal keys: the leftmost of every window


def test_sketch_refuses_parameters_out_of_range():
    for k, w in ((10, 10), (29, 10), (15, 0), (15, 65)):
        with pytest.raises(ValueError):
            M.sketch("ACGT" * 20, k, w)


# ---- chain -----------------------------------------------------------------------------------------------------------------------

def exhaustive_best(anchors, k, max_dist, bandwidth):
    """The largest score over ALL increasing subsets whose consecutive members satisfy the predecessor conditions, per end anchor."""
    def link(a, b):
        dr, dq = b[2] - a[2], b[3] - a[3]
        if a[0] != b[0] or a[1] != b[1] or not 0 < dq <= max_dist or not 0 < dr <= max_dist or abs(dr - dq) > bandwidth:
            return None
        return min(dq, dr, k) - M.cost(abs(dr - dq))
    n = len(anchors)
    best = [k] * n
    for size in range(2, n + 1):
        for sub in itertools.combinations(range(n), size):
            sc = k
            for a, b in zip(sub, sub[1:]):
                s = link(anchors[a], anchors[b])
                if s is None:
                    sc = None
                    break
                sc += s
            if sc is not None and sc > best[sub[-1]]:
                best[sub[-1]] = sc
    return best


@pytest.mark.parametrize("seed", range(6))
def test_chain_dp_equals_exhaustive_enumeration(seed):
    rng = random.Random(seed)
    n = rng.randint(6, 12)
    anchors = set()
    while len(anchors) < n:
        r = rng.randint(0, 400)
        anchors.add((rng.random() < 0.15, 0 if rng.random() < 0.85 else 1, r, max(0, r + rng.randint(-30, 30)) if rng.random() < 0.8
                     else rng.randint(0, 400)))
    anchors = sorted((int(s), c, r, q) for s, c, r, q in anchors)
    f, p = M.chain_dp(anchors, 15, 300, 25)
    assert f == exhaustive_best(anchors, 15, 300, 25)
    for i, j in enumerate(p):
        assert j < i and (j == -1) == (f[i] == 15)


def test_chain_tie_rules():
    # anchors 0 and 1 (no link between them: dq < 0) give anchor 2 the same score: the larger index wins
    anchors = [(0, 0, 100, 110), (0, 0, 110, 100), (0, 0, 200, 200)]
    f, p = M.chain_dp(anchors, 15, 5000, 500)
    assert M.cost(10) == 2 and f == [15, 15, 28] and p == [-1, -1, 1]
    anchors = [(0, 0, 100, 100), (0, 0, 100, 101), (0, 0, 130, 130)]
    f, p = M.chain_dp(anchors)
    assert f == [15, 15, 30] and p == [-1, -1, 1]                        # equal rpos is no predecessor; cost(1) = 0 makes 0 and 1 tie
    # a predecessor whose score only equals k is not taken, one above k is
    assert M.cost(7) == 2 and M.chain_dp([(0, 0, 100, 100), (0, 0, 102, 109)]) == ([15, 15], [-1, -1])
    assert M.cost(6) == 1 and M.chain_dp([(0, 0, 100, 100), (0, 0, 102, 108)]) == ([15, 16], [-1, 0])
    # two chains of equal score: the one that ends first is the primary, the other gives s2
    one = [(0, 0, 100, 100), (0, 0, 120, 120), (0, 0, 140, 140)]
    anchors = one + [(0, 0, r + 9000, q) for _, _, r, q in one]
    idx, s1, s2 = M.chain(anchors)
    assert idx == [0, 1, 2] and s1 == s2 == 45 and M.mapq_of(s1, s2, 3) == 0
    assert M.chain([]) == ([], 0, 0) and M.chain(one[:1]) == ([0], 15, 0)
    assert M.mapq_of(100, 0, 10) == 60 and M.mapq_of(100, 0, 9) == 30 and M.mapq_of(100, 50, 12) == 30
    assert [M.cost(g) for g in (0, 1, 2, 7, 32, 500)] == [0, 0, 0, 2, 7, 82]


def test_banded_pieces_equal_the_full_matrix():
    rng = random.Random(2)
    for _ in range(25):
        a = cases.random_seq(rng, rng.randint(0, 120))
        b = cases.mutate(rng, a, 0.3) if rng.random() < 0.7 else cases.random_seq(rng, rng.randint(0, 250))
        got = "".join("%d%s" % x for x in M.nw_ops(M.codes(a), M.codes(b)))
        if a and b:
            assert got == duplex_ref.nw(a, b)[1]
        else:
            assert got == ("%dI" % len(a) if a else "%dD" % len(b) if b else "")
    a = cases.random_seq(rng, 400)                                       # needs the band doubled: a long gap
    for b in (a[:100] + a[300:], cases.random_seq(rng, 180) + a):
        assert "".join("%d%s" % x for x in M.nw_ops(M.codes(a), M.codes(b))) == duplex_ref.nw(a, b)[1]


# ---- planted reads ---------------------------------------------------------------------------------------------------------------

def test_planted_reads_map_where_they_came_from():
    contigs, reads = cases.planted()
    expected = cases.planted_expected()
    assert len(reads) == 64 and sum(len(s) for _, s in contigs) == 50000
    assert {r[2] for r in reads} == {1, -1} and {r[1] for r in reads} == {0, 1}
    for rec, (seq, ci, strand, st, en) in zip(expected, reads):
        assert rec is not None
        assert rec["ctg"] == contigs[ci][0] and rec["strand"] == strand
        assert st - 50 <= rec["r_st"] and rec["r_en"] <= en + 50
        if len(seq) >= 1000:
            assert rec["q_en"] - rec["q_st"] >= 0.8 * len(seq)
        assert 0 <= rec["mapq"] <= 60
        cases.check_replay(rec, seq, contigs[ci][1])                     # NM, MD, mlen, blen by an independent walk


def test_reads_that_do_not_map():
    contigs, _ = cases.planted()
    index = M.Index(contigs)
    rng = random.Random(6)
    assert M.map_read(cases.random_seq(rng, 2000), index) is None
    assert M.map_read("ACGTACGTAC", index) is None and M.map_read("", index) is None


def test_non_acgt_reference_bases_count_as_mismatches():
    rng = random.Random(8)
    ref = cases.random_seq(rng, 3000)
    masked = ref[:1500] + "N" * 3 + ref[1503:]
    rec = M.map_read(ref[1000:2000], M.Index([("c", masked)]))
    assert rec["cigar_str"] == "1000M" and rec["NM"] == 3 and rec["MD"] == "500N0N0N497" and rec["mlen"] == 997
    cases.check_replay(rec, ref[1000:2000], masked)


def test_piece_cut_falls_behind_the_last_anchor_within_the_limit():
    k = 15
    q = np.zeros(40000, np.uint8)
    r = np.ones(40000, np.uint8)                                         # nothing to widen over
    anchors = [(100 + 1000 * i, 50 + 1000 * i) for i in range(36)]
    q_st, q_en, r_st, r_en, pieces = M.span_and_pieces(anchors, k, q, r)
    assert (q_st, q_en, r_st, r_en) == (36, 35051, 86, 35101)
    assert pieces == [(36, 16051, 86, 16101), (16051, 32051, 16101, 32101), (32051, 35051, 32101, 35101)]
    from bonito_amd import aligner
    got = aligner.span_and_pieces(np.array([a[0] for a in anchors]), np.array([a[1] for a in anchors]), k, q + 1, r + 2)
    assert got == (q_st, q_en, r_st, r_en, pieces)


# ---- host glue of the package ----------------------------------------------------------------------------------------------------

def test_host_finish_equals_the_restatement():
    from bonito_amd import aligner
    rng = random.Random(12)
    for _ in range(20):
        ref = cases.random_seq(rng, 300)
        ref = ref[:100] + "N" + ref[101:]
        read = cases.mutate(rng, ref[20:280], 0.15)
        q, r = M.codes(read), M.codes(ref)
        qa, ra = np.where(q > 3, 0, q), np.where(r > 3, 0, r)
        cut = len(read) // 2                                             # two pieces: equal ops merge at the seam
        ops = M.nw_ops(qa[:cut], ra[20:150]) + M.nw_ops(qa[cut:], ra[150:280])
        cigar = []
        for cnt, o in ops:
            op = {"=": 0, "X": 0, "I": 1, "D": 2}[o]
            if cigar and cigar[-1][1] == op:
                cigar[-1] = (cigar[-1][0] + cnt, op)
            else:
                cigar.append((cnt, op))
        nm, md, mlen, blen = M.finish(cigar, q, r, 0, 20)
        runs = np.array([(cnt << 2) | "=XID".index(o) for cnt, o in ops], np.uint32)
        got = aligner.finish(runs, aligner.encode(read), aligner.encode(ref), 0, 20)
        assert got == (cigar, "".join("%d%s" % (c, "MID"[o]) for c, o in cigar), nm, md, mlen, blen)
    assert aligner.finish(np.zeros(0, np.uint32), aligner.encode("ACGT"), aligner.encode("ACGT"), 0, 0) == ([], "", 0, "0", 0, 0)
    with pytest.raises(RuntimeError):                                    # runs that leave the read
        aligner.finish(np.array([(10 << 2) | 0], np.uint32), aligner.encode("ACGT"), aligner.encode("ACGTACGTACGT"), 0, 0)


def _golden():
    with open(os.path.join(GOLDEN, "mapper_sam_cases.json")) as fh:
        return json.load(fh)


def _mapping(m):
    if m is None:
        return None
    obj = types.SimpleNamespace(**m)
    obj.cigar = [tuple(c) for c in m["cigar"]]
    return obj


def test_sam_record_and_summary_row_equal_the_reference():
    from bonito_amd import io as bio
    g = _golden()
    read = types.SimpleNamespace(**g["read"])
    assert bio.summary_field_names + bio.alignment_field_names == g["field_names"]
    assert len(g["cases"]) == 12
    for case in g["cases"]:
        m = _mapping(case["mapping"])
        assert bio.sam_record(g["read"]["read_id"], g["sequence"], g["qstring"], m, tags=case["tags"]) == case["sam"], case["name"]
        assert bio.summary_row(read, len(g["sequence"]), g["qscore"], alignment=m) == case["summary"], case["name"]
    # without a mapping argument nothing changes
    assert bio.summary_row(read, 33, 12.5) == g["cases"][0]["summary"][:11]
    assert bio.sam_record("r", "ACGT", "!!!!") == "r\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t!!!!\tNM:i:0"


def test_sam_header_names_the_contigs_only_with_an_aligner():
    from bonito_amd import io as bio
    plain = bio.sam_header(["@RG\tID:x"])
    assert "@SQ" not in plain and "ID:aligner" not in plain and plain.count("\n") == 3
    al = types.SimpleNamespace(seq_names=["c1", "c2"], seq=lambda name: {"c1": "A" * 7, "c2": "C" * 11}[name])
    lines = bio.sam_header(["@RG\tID:x"], aligner=al).split("\n")
    assert lines[0].startswith("@HD") and lines[1:3] == ["@SQ\tSN:c1\tLN:7", "@SQ\tSN:c2\tLN:11"]
    assert lines[3].startswith("@PG\tID:basecaller") and lines[4].startswith("@PG\tID:aligner\tPN:bonito_amd") and lines[5] == "@RG\tID:x"


def test_fasta_parsing(tmp_path):
    from bonito_amd.aligner import Aligner, read_fasta
    text = ">chr1 first contig\nacgtAC\nGTnn\n\n>chr2\tother\nTTTT\n>empty\n"
    plain, gz = tmp_path / "ref.fa", tmp_path / "ref.fa.gz"
    plain.write_text(text)
    with gzip.open(gz, "wt") as fh:
        fh.write(text)
    want = [("chr1", "ACGTACGTNN"), ("chr2", "TTTT"), ("empty", "")]
    assert read_fasta(plain) == want and read_fasta(str(gz)) == want
    nothing = tmp_path / "nothing.fa"
    nothing.write_text("")
    al = Aligner(str(nothing))
    assert not al and al.seq_names == [] and al.map_batch(["ACGT" * 10]) == [None]
    with pytest.raises(ValueError, match="mmi"):
        Aligner(str(tmp_path / "ref.mmi"))
    with pytest.raises(ValueError):
        Aligner(str(nothing), k=10)


def test_align_map_keeps_the_order_and_flushes_the_last_batch():
    from bonito_amd.aligner import align_map
    calls = []

    class Fake:
        def map_batch(self, seqs):
            calls.append(len(seqs))
            return [None if len(s) % 2 else "m%d" % len(s) for s in seqs]

    stream = [("read%d" % i, {"sequence": "A" * i, "qstring": "!" * i}) for i in range(1, 18)]
    out = list(align_map(Fake(), iter(stream), batch=7))
    assert calls == [7, 7, 3] and [r for r, _ in out] == [r for r, _ in stream]
    assert [res["mapping"] for _, res in out] == [None if i % 2 else "m%d" % i for i in range(1, 18)]
    assert all(res["qstring"] == "!" * len(res["sequence"]) for _, res in out) and "mapping" not in stream[0][1]


def test_parser_refuses_reference_with_fasta(capsys):
    from bonito_amd.__main__ import main
    from bonito_amd.cli import basecaller
    args = basecaller.argparser().parse_args(["model", "reads", "--reference", "ref.fa", "--mm2-preset", "lr:hq", "--alignment-threads", "3"])
    assert args.reference == "ref.fa" and not args.sam and not args.fasta
    with pytest.raises(SystemExit):
        basecaller.argparser().parse_args(["model", "reads", "--reference", "ref.fa", "--fasta"])
    with pytest.raises(SystemExit):
        main(["basecaller", "model", "reads", "--fasta", "--reference", "ref.fa"])
    assert "not allowed with argument" in capsys.readouterr().err


def test_abi_refuses_bad_arguments_before_any_device_call():
    import ctypes as C
    from bonito_amd import _lib
    lib = _lib.lib()
    p = C.c_void_p(4096)                                                 # never read: every case is refused by the argument checks
    lens = np.array([100, 50], np.int32)
    hp = lens.ctypes.data_as(C.c_void_p)

    def sketch(k=15, w=10, lengths=hp, n=2, stride=128, ws=1 << 20, cap=1 << 20):
        rc = lib.bh_map_sketch(p, stride, lengths, n, k, w, p, ws, p, p, p, cap, p, None)
        return rc, _lib.last_error()
    for kw, word in ((dict(k=10), "k must be in 11..28"), (dict(k=29), "k must be in 11..28"), (dict(w=0), "w must be in 1..64"),
                     (dict(w=65), "w must be in 1..64"), (dict(ws=16), "workspace of 16 bytes"), (dict(cap=10), "may be needed"),
                     (dict(stride=64), "exceeds the row stride"), (dict(n=0), "n must be positive")):
        rc, msg = sketch(**kw)
        assert rc != 0 and word in msg, (kw, msg)
    neg = np.array([100, -1], np.int32)
    rc, msg = sketch(lengths=neg.ctypes.data_as(C.c_void_p))
    assert rc != 0 and "negative length" in msg
    big = np.array([(1 << 30) + 5, 1 << 30], np.int32)
    rc, msg = sketch(lengths=big.ctypes.data_as(C.c_void_p), stride=1 << 31, cap=1 << 40, ws=1 << 40)
    assert rc != 0 and "fewer than 2^31 bases" in msg
    assert lib.bh_map_sketch_workspace(2, 1 << 31) == 0 and lib.bh_map_sketch_workspace(2, 150) > 0
    assert lib.bh_map_sketch_tile() == 512
    rc = lib.bh_map_chain(p, p, p, 4, 100, 10, 5000, 500, p, p, p, p, None)
    assert rc != 0 and "k must be in 11..28" in _lib.last_error()
    rc = lib.bh_map_chain(p, p, p, 4, 1 << 31, 15, 5000, 500, p, p, p, p, None)
    assert rc != 0 and "fewer than 2^31" in _lib.last_error()
    rc = lib.bh_map_seed(p, p, p, p, p, 2000, 10, p, p, p, 5, p, p, 15, 64, p, None, None, 0, None)
    assert rc != 0 and "n must be in 1..1024" in _lib.last_error()

"""The device mapper (bonito_amd/aligner.py, csrc/mapper.hip) against its definition tests/mapper_ref.py: every comparison is on
integers or strings and exact."""
import io
import random
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import mapper_cases as cases
import mapper_ref as M

pytestmark = pytest.mark.gpu

QBITS, RBITS = 21, 31


def _aligner(contigs, **kw):
    from bonito_amd.aligner import Aligner
    return Aligner(list(contigs), **kw)


def _device_sketch(al, seqs):
    from bonito_amd.aligner import encode
    codes = [encode(s) for s in seqs]
    lens = np.array([len(c) for c in codes], np.int32)
    plane = np.zeros((len(seqs), max(1, int(lens.max()))), np.int8)
    for i, c in enumerate(codes):
        plane[i, :len(c)] = c
    keys, pos, strand, off = al._sketch(torch.from_numpy(plane).cuda(), plane.shape[1], lens)
    keys, pos, strand, off = keys.cpu().numpy(), pos.cpu().numpy(), strand.cpu().numpy(), off.cpu().numpy()
    return [list(zip(keys[off[i]:off[i + 1]].tolist(), pos[off[i]:off[i + 1]].tolist(), strand[off[i]:off[i + 1]].tolist()))
            for i in range(len(seqs))]


@pytest.fixture(scope="module")
def tiny():
    rng = random.Random(3)
    return [("a", cases.random_seq(rng, 400))]


@pytest.mark.parametrize("k,w", [(15, 10), (11, 1), (28, 64), (11, 64), (28, 1)])
def test_sketch_lengths_and_parameter_corners(tiny, k, w):
    from bonito_amd import _lib
    tile = _lib.lib().bh_map_sketch_tile()
    al = _aligner(tiny, k=k, w=w)
    rng = random.Random(100 * k + w)
    lengths = [0, k - 1, k, k + w - 2, k + w - 1, k + w, tile - 1, tile, tile + 1, tile + k + w - 2, 2 * tile - 1, 2 * tile, 2 * tile + 1,
               0, 5 * tile + 77]
    seqs = [cases.random_seq(rng, n) for n in lengths]
    got = _device_sketch(al, seqs)
    for s, g in zip(seqs, got):
        assert g == M.sketch(s, k, w), len(s)
    assert sum(len(g) for g in got) > 0


def test_sketch_corner_sequences(tiny):
    rng = random.Random(5)
    unit = cases.random_seq(rng, 37)
    r = cases.random_seq(rng, 1500)
    seqs = ["A" * 700,                                   # a homopolymer: one key everywhere, the leftmost of each window
            unit * 30,                                   # an exact tandem repeat: equal keys a period apart
            "ACGT" * 200, "AT" * 300,                    # every fourth 12-mer / every even k-mer is its own reverse complement
            r[:300] + "N" * 5 + r[300:700] + "N" * 40 + r[700:] + "N",
            "N" * 100, "", r, "", "ACGTN" * 3]
    for k, w in ((15, 10), (12, 5)):
        al = _aligner(tiny, k=k, w=w)
        got = _device_sketch(al, seqs)
        for s, g in zip(seqs, got):
            assert g == M.sketch(s, k, w), (k, w, s[:20], len(s))
    assert M.sketch("AT" * 300, 12, 5) == [] and len(M.sketch("A" * 700, 15, 10)) > 60


def test_index_is_the_sorted_table():
    contigs, _ = cases.planted()
    al = _aligner(contigs)
    ref = M.Index(contigs)
    assert al.index_keys.cpu().tolist() == [t[0] for t in ref.table]
    starts = [0, len(contigs[0][1])]
    assert al._rpos.cpu().tolist() == [starts[t[1]] + t[2] for t in ref.table]
    assert al._rstrand.cpu().tolist() == [t[3] for t in ref.table]


def _unpack(words, starts):
    out = []
    for v in words:
        g = (v >> QBITS) & ((1 << RBITS) - 1)
        ci = max(i for i, s in enumerate(starts) if s <= g)
        out.append((v >> (QBITS + RBITS + 1), ((v >> (QBITS + RBITS)) & 1, ci, g - starts[ci], v & ((1 << QBITS) - 1))))
    return out


def _device_anchors(al, reads, starts):
    words, _ = al.anchors_of(reads)
    per = [[] for _ in reads]
    for read, a in _unpack(words.cpu().tolist(), starts):
        per[read].append(a)
    return per


def test_seed_occurrence_limit_and_hits():
    rng = random.Random(9)
    u, v = cases.random_seq(rng, 60), cases.random_seq(rng, 60)
    body = "".join(cases.random_seq(rng, 50) + (u if i < 4 else "") + cases.random_seq(rng, 30) + v for i in range(5))
    contigs = [("r1", body + cases.random_seq(rng, 300)), ("r2", cases.random_seq(rng, 500))]
    starts = [0, len(contigs[0][1])]
    al, ref = _aligner(contigs, max_occ=4), M.Index(contigs, max_occ=4)
    counts = sorted(len(o) for o in ref.occ.values())
    assert 4 in counts and 5 in counts                                   # keys with exactly max_occ and max_occ + 1 occurrences
    reads = [u, v, M.revcomp(u), cases.random_seq(rng, 300), contigs[1][1][100:400], "", u + cases.random_seq(rng, 40) + v]
    got = _device_anchors(al, reads, starts)
    want = [M.seed(M.sketch(s, 15, 10), len(s), ref) for s in reads]
    assert got == want
    assert len(want[0]) >= 4 and want[1] == [] and want[3] == [] and all(a[0] == 1 for a in want[2])
    assert len(want[4]) == len(M.sketch(reads[4], 15, 10))               # every minimizer of an exact copy hits


def _pack(read, anchors, starts):
    return [(read << (QBITS + RBITS + 1)) | (st << (QBITS + RBITS)) | ((starts[ci] + r) << QBITS) | q for st, ci, r, q in anchors]


def _colinear(rng, n, st=0, ci=0, r0=1000, q0=50):
    out, r, q = [], r0, q0
    for _ in range(n):
        out.append((st, ci, r, q))
        step = rng.randint(1, 40)
        r, q = r + step + (rng.randint(-3, 3) if rng.random() < 0.3 else 0), q + step
    return sorted(set(out))


def _chain_cases():
    rng = random.Random(17)
    k, md, bw = 15, 5000, 500
    c = {}
    for n in (0, 1, 2, 63, 64, 65, 129):
        c["n%d" % n] = _colinear(rng, n)
    noisy = _colinear(rng, 2600) + [(0, 0, rng.randint(1000, 60000), rng.randint(0, 60000)) for _ in range(400)]
    c["n3000"] = sorted(set(noisy))
    c["both_strands"] = sorted(set(_colinear(rng, 40) + _colinear(rng, 70, st=1, r0=5000)))
    c["two_contigs"] = sorted(set(_colinear(rng, 30, ci=0, r0=60000) + _colinear(rng, 90, ci=1, r0=10, q0=20)))
    c["equal_rpos"] = [(0, 0, 100, 20), (0, 0, 100, 30), (0, 0, 100, 45), (0, 0, 130, 50), (0, 0, 130, 75), (0, 0, 160, 80)]
    base = [(0, 0, 100 + 20 * i, 100 + 20 * i) for i in range(10)]       # f = 150 at its end: a jump of 500 (cost 82) is still taken
    c["band_edge"] = base + [(0, 0, 300 + bw, 300), (0, 0, 320 + 2 * bw + 1, 320)]
    c["dist_edge"] = base + [(0, 0, 280 + md, 280 + md), (0, 0, 281 + 2 * md, 281 + 2 * md)]
    # equal scores: two predecessors of the last anchor tie (the larger index wins); two chain ends tie (the smaller index wins)
    c["ties"] = [(0, 0, 100, 100), (0, 0, 101, 101), (0, 0, 130, 130), (0, 0, 9000, 100), (0, 0, 9001, 101), (0, 0, 9030, 130)]
    c["empty_between"] = []
    return c


def test_chain_matches_the_restatement():
    contigs = [("a", "A" * 80000), ("b", "C" * 70000)]
    starts = [0, 80000]
    al = _aligner(contigs)
    named = _chain_cases()
    order = ["n129", "empty_between", "n3000", "n0", "n1", "n2", "n63", "n64", "n65", "both_strands", "two_contigs", "equal_rpos",
             "band_edge", "dist_edge", "ties", "n0", "both_strands"]
    words = []
    for read, name in enumerate(order):
        packed = _pack(read, named[name], starts)
        assert packed == sorted(packed)                                  # the word order is the tuple order
        words += packed
    dev = torch.tensor(words, dtype=torch.int64, device="cuda")
    off, contig, f, p, chain, result = (t.cpu().numpy() for t in al._chain(dev, len(order)))
    for read, name in enumerate(order):
        anchors = named[name]
        a0, a1 = int(off[read]), int(off[read + 1])
        assert a1 - a0 == len(anchors)
        wf, wp = M.chain_dp(anchors)
        assert f[a0:a1].tolist() == wf and p[a0:a1].tolist() == wp, name
        idx, s1, s2 = M.chain(anchors)
        cnt, g1, g2, end = result[read].tolist()
        assert (cnt, g1, g2) == (len(idx), s1, s2), name
        assert chain[a0:a0 + cnt][::-1].tolist() == idx and end == (idx[-1] if idx else -1), name
    # at the bandwidth / at max_dist the predecessor is taken, one beyond it is not
    assert M.chain_dp(named["band_edge"])[1][10:] == [9, -1] and M.chain_dp(named["dist_edge"])[1][10:] == [9, -1]
    assert M.chain(named["both_strands"])[2] > 0 and M.chain(named["two_contigs"])[2] > 0


def _same(got, want):
    assert (got is None) == (want is None)
    if want is not None:
        assert got.as_dict() == want


def test_map_batch_planted_set_equals_the_restatement():
    contigs, reads = cases.planted()
    want = cases.planted_expected()
    al = _aligner(contigs)
    rng = random.Random(1)
    extra = [cases.random_seq(rng, 1500), "ACGTACGT", ""]                # not from the reference, shorter than k, empty
    got = al.map_batch([r[0] for r in reads] + extra)
    assert len(got) == len(reads) + 3 and got[-3:] == [None, None, None]
    for g, w_, (seq, ci, strand, st, en) in zip(got, want, reads):
        _same(g, w_)
        assert g.ctg == contigs[ci][0] and g.strand == strand and st - 50 <= g.r_st and g.r_en <= en + 50
        cases.check_replay(g, seq, contigs[ci][1])
    assert al.map_batch([r[0].lower() for r in reads[:2]])[1].as_dict() == want[1]


def test_map_batch_long_read_crosses_the_piece_cut():
    rng = random.Random(77)
    contigs = [("long", cases.random_seq(rng, 76000))]
    read = M.revcomp(cases.mutate(rng, contigs[0][1][3000:73000], 0.02))
    assert len(read) > 4 * M.PIECE
    want = M.map_read(read, M.Index(contigs))
    got = _aligner(contigs).map_batch([read])[0]
    _same(got, want)
    assert got.strand == -1 and got.q_en - got.q_st > 0.95 * len(read)
    cases.check_replay(got, read, contigs[0][1])


def test_map_batch_read_over_a_contig_boundary_maps_inside_one_contig():
    contigs, _ = cases.planted()
    a, b = contigs[0][1], contigs[1][1]
    read = a[-900:] + b[:600]
    al = _aligner(contigs)
    got = al.map_batch([read])[0]
    _same(got, M.map_read(read, M.Index(contigs)))
    assert got.ctg == "ctgA" and got.r_en <= len(a) and got.q_en <= 900
    cases.check_replay(got, read, a)


def _pairs(reads):
    out = []
    for i, (seq, *_rest) in enumerate(reads):
        read = types.SimpleNamespace(read_id="read_%d" % i, filename="f%d.pod5" % i, run_id="run", channel=1, mux=2, start=0.5,
                                     duration=1.5, template_start=0.5, template_duration=1.5, num_samples=4000, trimmed_samples=10,
                                     signal=np.zeros(3990, np.float32))
        out.append((read, {"sequence": seq, "qstring": "5" * len(seq), "stride": 5, "moves": np.zeros(0, np.int8)}))
    return out


def test_align_map_through_the_writer(tmp_path):
    from bonito_amd import io as bio
    from bonito_amd.aligner import align_map
    contigs, reads = cases.planted()
    rng = random.Random(4)
    reads = list(reads[:15]) + [(cases.random_seq(rng, 800), 0, 1, 0, 0)]          # 16 reads in batches of 7: 7 + 7 + 2
    al = _aligner(contigs)
    fd, summary = io.StringIO(), tmp_path / "summary.tsv"
    writer = bio.Writer("sam", align_map(al, iter(_pairs(reads)), batch=7), fd=fd, summary_path=str(summary), aligner=al)
    writer.start()
    writer.join()
    assert writer.error is None
    lines = fd.getvalue().strip().split("\n")
    header, records = [l for l in lines if l.startswith("@")], [l.split("\t") for l in lines if not l.startswith("@")]
    assert header[1:3] == ["@SQ\tSN:ctgA\tLN:30000", "@SQ\tSN:ctgB\tLN:20000"] and any(l.startswith("@PG\tID:aligner") for l in header)
    assert [r[0] for r in records] == ["read_%d" % i for i in range(16)]
    rows = [l.split("\t") for l in summary.read_text().strip().split("\n")]
    assert rows[0] == bio.summary_field_names + bio.alignment_field_names and len(rows) == 17
    names = dict(contigs)
    for rec, row, (seq, ci, strand, st, en) in zip(records[:15], rows[1:], reads):
        assert rec[1] == ("0" if strand == 1 else "16") and rec[2] == contigs[ci][0]
        assert rec[9] == (seq if strand == 1 else M.revcomp(seq))
        cigar = rec[5]
        clips = re.findall(r"(\d+)S", cigar)
        core = re.sub(r"\d+S", "", cigar)
        q_st = int(re.match(r"(\d+)S", cigar).group(1)) if re.match(r"\d+S", cigar) else 0      # on the record's (aligned) strand
        fake = dict(strand=1, q_st=q_st, r_st=int(rec[3]) - 1, cigar_str=core)
        nm, md, mlen, blen, dq, dr = cases.replay(fake, rec[9], names[rec[2]])
        assert rec[11] == "NM:i:%d" % nm and rec[12] == "MD:Z:%s" % md
        assert q_st + dq + (int(clips[-1]) if cigar.endswith("S") else 0) == len(seq)
        assert row[11] == rec[2] and int(row[12]) == int(rec[3]) - 1 and int(row[13]) == int(rec[3]) - 1 + dr
        assert row[16] == ("+" if strand == 1 else "-") and int(row[17]) == blen and int(row[19]) == mlen
    assert records[15][1:6] == ["4", "*", "0", "0", "*"] and rows[16][11:17] == ["*", "-1", "-1", "-1", "-1", "*"]


def test_cli_reference_writes_aligned_sam_and_two_ranks_write_the_same_bytes(tmp_path):
    from conftest import ROOT
    from test_gpu_basecall import _write_model_dir
    mdir, rdir = tmp_path / "model", tmp_path / "reads"
    mdir.mkdir(); rdir.mkdir()
    _write_model_dir(mdir, fixture="lstm96_sl3")
    rng = np.random.default_rng(8)
    for i in range(9):
        np.save(rdir / ("read%d.npy" % i), (rng.standard_normal(int(rng.integers(700, 9000))) * 12 + 90).astype(np.float32))
    contigs, _ = cases.planted()
    ref = tmp_path / "ref.fa"
    ref.write_text("".join(">%s some description\n%s\n" % (n, "\n".join(s[i:i + 70] for i in range(0, len(s), 70))) for n, s in contigs))
    outs = []
    for extra in ([], ["--devices", "0,0"]):
        summ = tmp_path / ("summary%d.tsv" % len(outs))
        r = subprocess.run([sys.executable, "-m", "bonito_amd", "basecaller", str(mdir), str(rdir), "--summary", str(summ),
                            "--batchsize", "8", "--reference", str(ref)] + extra, capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(("\n".join(l for l in r.stdout.split("\n") if not l.startswith("@PG\tID:basecaller")), summ.read_text()))
    assert outs[0] == outs[1]
    lines = outs[0][0].strip().split("\n")
    assert lines[0].startswith("@HD") and lines[1:3] == ["@SQ\tSN:ctgA\tLN:30000", "@SQ\tSN:ctgB\tLN:20000"]
    records = [l.split("\t") for l in lines if not l.startswith("@")]
    assert len(records) == 9
    names = dict(contigs)
    for rec in records:
        if rec[1] == "4":
            assert rec[2:9] == ["*", "0", "0", "*", "*", "0", "0"]
        else:
            lead = re.match(r"(\d+)S", rec[5])
            fake = dict(strand=1, q_st=int(lead.group(1)) if lead else 0, q_en=len(rec[9]), r_st=int(rec[3]) - 1, cigar_str=re.sub(r"\d+S", "", rec[5]))
            nm, md = cases.replay(fake, rec[9], names[rec[2]])[:2]
            assert rec[11] == "NM:i:%d" % nm and rec[12] == "MD:Z:%s" % md
    assert outs[0][1].split("\n")[0].split("\t")[11] == "alignment_genome"

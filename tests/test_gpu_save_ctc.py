"""``basecaller --save-ctc`` and ``--reference --extend-ends`` end to end on the GPU: reads are cut into chunks and basecalled once
in-process, a reference is built FROM those calls (copied, reverse-complemented, with a substitution near an end, mutated, left out),
and the command line must then turn the same reads and that reference into exactly the training set the plan predicts.

One deviation from the letter of the plan: the label of a chunk whose copy in the reference carries a substitution is that copy (the
reference under the alignment), not the call - it equals the call in every base but the substituted one, and it has the call's full
length only because the alignment is extended over the substitution to the end of the call."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import mapper_cases as cases
import mapper_ref as M

pytestmark = pytest.mark.gpu

CHUNKSIZE, OVERLAP, BATCHSIZE = 2400, 0, 8
EXACT, MINUS, NEAR_END, MUTATED, LEFT_OUT = range(5)
PLAN = (EXACT, MINUS, NEAR_END, MUTATED, LEFT_OUT, EXACT, NEAR_END, MINUS)          # the treatment of chunk k is PLAN[k % 8]
NEXT = str.maketrans("ACGT", "CGTA")


def _treat(call, kind, k):
    """-> the piece of the reference that stands for this call, as it reads on the call's strand (None: left out)"""
    if kind == LEFT_OUT:
        return None
    if kind == NEAR_END:                                                  # five matching bases, then the substitution, from one end
        at = 5 if k % 3 == 0 else len(call) - 6
        # a base that neither the call nor its neighbours have there: in a homopolymer any other choice could be explained as well
        # by an insertion, and the label would lose a base to the rule that the shorter of two equal extensions is taken
        other = next(b for b in "ACGT" if b not in call[at - 1:at + 2])
        return call[:at] + other + call[at + 1:]
    if kind == MUTATED:                                                   # every tenth base of the middle half: 5 % in all
        lo, hi = len(call) // 4, len(call) - len(call) // 4
        return "".join(c.translate(NEXT) if lo <= i < hi and i % 10 == 0 else c for i, c in enumerate(call))
    return call


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from test_gpu_basecall import _write_model_dir
    from bonito_amd import util
    from bonito_amd.nn import fuse_bn_
    from bonito_amd.reader import Reader, read_chunks
    tmp = tmp_path_factory.mktemp("save_ctc")
    mdir, rdir = tmp / "model", tmp / "reads"
    mdir.mkdir(); rdir.mkdir()
    _write_model_dir(mdir, fixture="lstm96_sl3", batchsize=BATCHSIZE, chunksize=CHUNKSIZE, overlap=OVERLAP)
    # The fixture's random weights as they stand ignore the signal: the recurrent stack sits at a fixed point and every chunk is called
    # CACACA..., which no chunk length makes mappable. The weights that carry the signal forward are scaled up (input weights of the
    # recurrent layers x 8, convolutions x 3) and the head's gain is taken from 30 to 10 so that blanks occur and the calls differ in
    # length: calls of about 350 bases per chunk in which nearly every 15-mer is new (seen with the CPU oracle of the same model).
    import torch
    sd = torch.load(str(mdir / "weights_1.tar"))
    for key in sd:
        if key.endswith("weight_ih_l0"):
            sd[key] = sd[key] * 8.0
        elif key.endswith("conv.weight"):
            sd[key] = sd[key] * 3.0
        elif key.endswith("linear.weight"):
            sd[key] = sd[key] / 3.0
    torch.save(sd, str(mdir / "weights_1.tar"))
    rng = np.random.default_rng(14)
    for i, n in enumerate([2500, 4900, 5100, 2411, 7300, 4811, 2600, 5000, 4850, 2450, 5300, 3000]):
        np.save(rdir / ("read%02d.npy" % i), (rng.standard_normal(n) * 12 + 90).astype(np.float32))
    model = util.load_model(str(mdir), "cuda", use_koi=True).apply(fuse_bn_)
    basecall = util.load_symbol(str(mdir), "basecall")
    bc = model.config["basecaller"]
    assert (bc["chunksize"], bc["overlap"], bc["batchsize"]) == (CHUNKSIZE, OVERLAP, BATCHSIZE)
    reads = Reader(str(rdir)).get_reads(scaling_strategy=model.config.get("scaling"), norm_params=model.config.get("normalisation"))
    chunks = [c for read in reads for c in read_chunks(read, chunksize=CHUNKSIZE, overlap=OVERLAP)]
    called = list(basecall(model, iter(chunks), batchsize=BATCHSIZE, chunksize=CHUNKSIZE, overlap=OVERLAP))
    assert [c.read_id for c, _ in called] == [c.read_id for c in chunks] and len(chunks) >= 16
    calls = {c.read_id: res["sequence"] for c, res in called}
    print("chunks %d, call lengths %s" % (len(chunks), sorted(len(s) for s in calls.values())))
    assert min(len(s) for s in calls.values()) >= 150                     # long enough to chain, and one substitution keeps 0.99
    # the reference: the treated calls in a shuffled order on three contigs, random spacers between them, none at the contigs' ends
    py = random.Random(31)
    pieces = {}
    for k, c in enumerate(chunks):
        piece = _treat(calls[c.read_id], PLAN[k % len(PLAN)], k)
        if piece is not None:
            pieces[c.read_id] = (piece, PLAN[k % len(PLAN)])
    order = sorted(pieces)
    py.shuffle(order)
    contigs = []
    for x in range(3):
        parts = []
        for rid in order[x::3]:
            piece, kind = pieces[rid]
            parts.append(M.revcomp(piece) if kind == MINUS else piece)
        contigs.append(("ctg%d" % x, "".join(p + (cases.random_seq(py, py.randint(60, 200)) if i + 1 < len(parts) else "")
                                             for i, p in enumerate(parts))))
    # the plan holds only if a call that was left out resembles no other call (the restatement of the mapper finds nothing for it)
    # and a mutated one is still found
    index = M.Index(contigs)
    for k, c in enumerate(chunks):
        kind = PLAN[k % len(PLAN)]
        if kind in (LEFT_OUT, MUTATED):
            assert (M.map_read(calls[c.read_id], index) is None) == (kind == LEFT_OUT), (c.read_id, kind)
    ref = tmp / "ref.fa"
    ref.write_text("".join(">%s planted calls\n%s\n" % (n, "\n".join(s[i:i + 70] for i in range(0, len(s), 70))) for n, s in contigs))
    signals = {c.read_id: np.array(c.signal, dtype=np.float16) for c in chunks}
    return dict(tmp=tmp, mdir=mdir, rdir=rdir, ref=ref, contigs=contigs, chunks=[c.read_id for c in chunks], calls=calls, pieces=pieces,
                signals=signals)


def _cli(world, *extra, summary):
    from conftest import ROOT
    r = subprocess.run([sys.executable, "-m", "bonito_amd", "basecaller", str(world["mdir"]), str(world["rdir"]), "--summary", str(summary),
                        "--reference", str(world["ref"]), "--seed", "3", *extra], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return r


def _load(directory):
    return tuple(np.load(os.path.join(directory, name)) for name in ("chunks.npy", "references.npy", "reference_lengths.npy"))


def test_save_ctc_writes_the_planted_training_set(world, capsys):
    tmp = world["tmp"]
    runs = []
    for name in ("a", "b"):
        out = tmp / ("ctc_" + name)
        r = _cli(world, "--save-ctc", "--ctc-output-dir", str(out), summary=tmp / ("summary_%s.tsv" % name))
        runs.append((r, out))
    r, out = runs[0]
    chunks, refs, lens = _load(out)
    assert chunks.dtype == np.float16 and refs.dtype == np.uint8 and lens.dtype == np.uint16
    n = len(lens)
    assert chunks.shape == (n, CHUNKSIZE) and refs.shape[0] == n and lens.shape == (n,)
    # what the plan predicts: every chunk but the mutated and the left-out ones is accepted, with its piece of the reference as label
    kinds = [PLAN[k % len(PLAN)] for k in range(len(world["chunks"]))]
    accepted = [rid for rid, kind in zip(world["chunks"], kinds) if kind in (EXACT, MINUS, NEAR_END)]
    counts = dict(re.findall(r"^ - (\S+): (\d+)$", r.stderr, flags=re.M))
    print("rejected %s, accepted %d of %d, written %d" % (counts, len(accepted), len(kinds), n))
    assert counts == {"low_accuracy0.99": str(kinds.count(MUTATED)), "no_mapping": str(kinds.count(LEFT_OUT))}
    label_len = np.array([len(world["pieces"][rid][0]) for rid in accepted])
    mu, sd = label_len.mean(), label_len.std()
    typical = [rid for rid, m in zip(accepted, label_len) if mu - 2.5 * sd < m < mu + 2.5 * sd]
    assert n == len(typical) >= 8 and refs.shape[1] == label_len.max()
    rows = [l.split("\t") for l in (tmp / "summary_a.tsv").read_text().strip().split("\n")]
    assert rows[0][1] == "read_id" and rows[0][11] == "alignment_genome" and len(rows) == n + 1
    assert sorted(row[1] for row in rows[1:]) == sorted(typical) and [row[1] for row in rows[1:]] != typical      # shuffled
    near_end = minus = 0
    for k, row in enumerate(rows[1:]):
        rid = row[1]
        piece, kind = world["pieces"][rid]
        call = world["calls"][rid]
        label = "".join(" ACGT"[x] for x in refs[k, :lens[k]])
        assert label == piece and (refs[k, lens[k]:] == 0).all(), (rid, kind)
        assert len(label) == len(call) and sum(a != b for a, b in zip(label, call)) == (1 if kind == NEAR_END else 0)
        assert np.array_equal(chunks[k], world["signals"][rid])
        assert row[16] == ("-" if kind == MINUS else "+")
        near_end += kind == NEAR_END
        minus += kind == MINUS
    assert near_end >= 2 and minus >= 2
    assert "  - chunks.npy with shape (%d,%d)\n" % (n, CHUNKSIZE) in r.stderr and "> written ctc training data to %s\n" % out in r.stderr
    # the SAM stream on stdout: one record per accepted chunk, in the order of the chunks
    records = [l.split("\t") for l in r.stdout.split("\n") if l and not l.startswith("@")]
    assert [rec[0] for rec in records] == accepted
    assert r.stdout.count("@SQ\tSN:ctg") == 3
    # the same seed, the same bytes
    for name in ("chunks.npy", "references.npy", "reference_lengths.npy"):
        assert (out / name).read_bytes() == (runs[1][1] / name).read_bytes(), name
    assert (tmp / "summary_a.tsv").read_bytes() == (tmp / "summary_b.tsv").read_bytes()
    # evaluate reads the directory and scores every chunk of it
    from bonito_amd.__main__ import main
    capsys.readouterr()
    assert main(["evaluate", str(world["mdir"]), "--directory", str(out), "--weights", "1", "--batchsize", "8"]) == 0
    text = capsys.readouterr().out
    assert re.search(r"^\* num_chunks\s+%d$" % n, text, flags=re.M) and "* loss mean" in text and "* accuracy" in text


def _clips(cigar):
    lead, trail = re.match(r"(\d+)S", cigar), re.search(r"(\d+)S$", cigar)
    return int(lead.group(1)) if lead else 0, int(trail.group(1)) if trail else 0


def test_extend_ends_only_shortens_the_soft_clips_of_the_sam_records(world):
    tmp = world["tmp"]
    plain = _cli(world, summary=tmp / "summary_plain.tsv")
    ext = _cli(world, "--extend-ends", summary=tmp / "summary_ext.tsv")
    names = dict(world["contigs"])
    both = []
    for r in (plain, ext):
        records = [l.split("\t") for l in r.stdout.split("\n") if l and not l.startswith("@")]
        assert len(records) == 12
        for rec in records:
            if rec[1] != "4":
                lead = _clips(rec[5])[0]
                fake = dict(strand=1, q_st=lead, q_en=len(rec[9]), r_st=int(rec[3]) - 1, cigar_str=re.sub(r"\d+S", "", rec[5]))
                nm, md, _mlen, _blen, dq, _dr = cases.replay(fake, rec[9], names[rec[2]])
                assert rec[11] == "NM:i:%d" % nm and rec[12] == "MD:Z:%s" % md and lead + dq + _clips(rec[5])[1] == len(rec[9])
        both.append(records)
    mapped = shorter = 0
    for old, new in zip(*both):
        assert old[:3] == new[:3] and old[4] == new[4] and old[9] == new[9]       # the same read, strand, contig, mapq and bases
        if old[1] == "4":
            continue
        mapped += 1
        (a0, a1), (b0, b1) = _clips(old[5]), _clips(new[5])
        assert b0 <= a0 and b1 <= a1
        shorter += b0 + b1 < a0 + a1
    print("mapped %d of 12, shorter clips in %d" % (mapped, shorter))
    assert mapped >= 6 and shorter >= 1

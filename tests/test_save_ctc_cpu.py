"""``basecaller --save-ctc`` on the host: ``reader.read_chunks``, ``io.CTCWriter`` fed with made-up (chunk, result) streams and a made-up
aligner, and the parser's refusals. No GPU."""
import io
import json
import os
import types

import numpy as np
import pytest

from conftest import GOLDEN


def _read(n, **kw):
    base = dict(read_id="7d5a3c1e-read", run_id="run_a1", filename="batch_0.pod5", mux=3, channel=12, start=101.25, duration=2.5)
    base.update(kw)
    return types.SimpleNamespace(signal=np.arange(n, dtype=np.float32), **base)


# ---- read_chunks -----------------------------------------------------------------------------------------------------------------

def test_read_chunks_lengths_ids_and_slices():
    from bonito_amd.reader import ReadChunk, read_chunks
    cs, ov = 1000, 100
    step = cs - ov
    for n in (0, cs - 1):
        assert list(read_chunks(_read(n), cs, ov)) == []
    for n in (cs, cs + 1, cs + step - 1, cs + step, cs + step + 1, cs + 2 * step, cs + 2 * step + 1, 5 * cs + 37):
        read = _read(n)
        chunks = list(read_chunks(read, chunksize=cs, overlap=ov))
        count, offset = (n - cs) // step + 1, (n - cs) % step
        assert len(chunks) == count and [c.read_id for c in chunks] == ["7d5a3c1e-read:%d:%d" % (i + 1, count) for i in range(count)]
        for i, c in enumerate(chunks):
            assert isinstance(c, ReadChunk) and c.signal.dtype == np.float32 and len(c.signal) == cs
            assert np.array_equal(c.signal, read.signal[offset + i * step:offset + i * step + cs])
            assert np.shares_memory(c.signal, read.signal)                # a view, not a copy
        assert chunks[-1].signal[-1] == n - 1                              # the last chunk ends with the signal
        c = chunks[0]
        assert (c.run_id, c.filename, c.mux, c.channel, c.start, c.duration) == ("run_a1", "batch_0.pod5", 3, 12, 101.25, 2.5)
        assert (c.template_start, c.template_duration) == (101.25, 2.5) and repr(c) == "ReadChunk('7d5a3c1e-read:1:%d')" % count


def test_read_chunks_equal_the_reference():
    """tests/golden/read_chunks_cases.json: recorded from the reference's own read_chunks (make_golden_read_chunks.py)"""
    from bonito_amd.reader import read_chunks
    with open(os.path.join(GOLDEN, "read_chunks_cases.json")) as fh:
        g = json.load(fh)
    assert len(g["cases"]) == 15
    for case in g["cases"]:
        chunks = list(read_chunks(_read(case["length"], **g["read"]), chunksize=case["chunksize"], overlap=case["overlap"]))
        assert [c.read_id for c in chunks] == case["ids"], case
        assert [int(c.signal[0]) for c in chunks] == case["first"] and [len(c.signal) for c in chunks] == case["sizes"]
        got = [[c.run_id, c.filename, c.mux, c.channel, c.start, c.duration, c.template_start, c.template_duration] for c in chunks[:1]]
        assert got == case["fields"]


# ---- CTCWriter -------------------------------------------------------------------------------------------------------------------

CONTIG = "ACGTTGCAAGGCTTAACCGGTATCGATTGCAGTCCATGGACTAGCTAGGATCCAGTNACGGTACCTTAGGCATCGA"
COMP = str.maketrans("ACGT", "TGCA")


class FakeAligner:
    seq_names = ["chr1", "other"]

    def seq(self, name, start=0, end=None):
        return {"chr1": CONTIG, "other": "ACGT" * 5}[name][start:end]


def _mapping(r_st, r_en, strand=1, q_st=0, q_en=None, mlen=None, blen=None):
    n = r_en - r_st
    return types.SimpleNamespace(ctg="chr1", r_st=r_st, r_en=r_en, q_st=q_st, q_en=n if q_en is None else q_en, strand=strand, mapq=60,
                                 cigar=[(n, 0)], cigar_str="%dM" % n, NM=0, MD=str(n), mlen=n if mlen is None else mlen,
                                 blen=n if blen is None else blen)


def _chunk(i, size=16):
    return types.SimpleNamespace(read_id="read:%d:9" % i, run_id="run", filename="f.pod5", mux=1, channel=2, start=0.5, duration=1.5,
                                 template_start=0.5, template_duration=1.5, signal=np.full(size, i, np.float32) + np.arange(size) / 64)


def _call(m, qstring=None, seq=None):
    seq = seq if seq is not None else (CONTIG[m.r_st:m.r_en] if m.strand == 1 else CONTIG[m.r_st:m.r_en].translate(COMP)[::-1])
    return {"sequence": seq, "qstring": qstring if qstring is not None else "5" * len(seq), "mapping": m}


def _run(stream, tmp_path, seed=7, **kw):
    from bonito_amd import io as bio
    fd = io.StringIO()
    os.makedirs(tmp_path, exist_ok=True)
    np.random.seed(seed)
    writer = bio.CTCWriter("sam", iter(stream), FakeAligner(), fd=fd, summary_path=str(tmp_path / "summary.tsv"),
                           output_directory=str(tmp_path / "ctc"), **kw)
    writer.start()
    writer.join()
    assert writer.error is None
    return writer, fd.getvalue()


def test_ctc_writer_counts_every_reject_reason_once(tmp_path, capsys):
    from bonito_amd import io as bio
    good = [_mapping(0, 20), _mapping(2, 23), _mapping(5, 27, strand=-1), _mapping(30, 52)]
    stream = [(_chunk(i), _call(m)) for i, m in enumerate(good)]
    stream.insert(1, (_chunk(10), _call(_mapping(0, 20), qstring="#" * 20)))                     # Q2 < 5
    stream.insert(2, (_chunk(11), {"sequence": "", "qstring": "", "mapping": None}))              # nothing called (mean q-score 0)
    stream.insert(3, (_chunk(12), {"sequence": "ACGT" * 5, "qstring": "5" * 20, "mapping": None}))
    stream.insert(4, (_chunk(13), _call(_mapping(0, 20, mlen=19, blen=20))))                     # 0.95 < 0.99
    stream.insert(5, (_chunk(14), _call(_mapping(0, 20, q_st=1, q_en=18), seq=CONTIG[:20])))     # 17 / 20 < 0.90
    stream.insert(6, (_chunk(15), _call(_mapping(45, 65))))                                      # the contig's N
    writer, sam = _run(stream, tmp_path, min_qscore=5.0)
    assert dict(writer.rejected) == {"low_qscore": 2, "no_mapping": 1, "low_accuracy0.99": 1, "low_coverage0.90": 1, "N_in_sequence": 1}
    # with no q-score bar the empty call is counted for what it is
    writer2, _ = _run(stream, tmp_path / "again", min_qscore=0.0)
    assert dict(writer2.rejected) == {"zerolen_sequence": 1, "no_mapping": 1, "low_accuracy0.99": 1, "low_coverage0.90": 1, "N_in_sequence": 1}
    assert len(writer.log) == 10 and writer.log[0] == ("read:0:9", 16)
    err = capsys.readouterr().err
    assert "> Chunks rejected from training data:\n - low_qscore: 2\n - no_mapping: 1\n - low_accuracy0.99: 1\n" in err
    assert "  - chunks.npy with shape (4,16)\n  - references.npy with shape (4,22)\n  - reference_lengths.npy shape (4)\n" in err
    assert "> written ctc training data to %s\n" % (tmp_path / "ctc") in err
    # the SAM stream: the header with the aligner's contigs, then the accepted chunks in the order they came, as io.sam_record writes them
    lines = sam.strip().split("\n")
    assert lines[1:3] == ["@SQ\tSN:chr1\tLN:%d" % len(CONTIG), "@SQ\tSN:other\tLN:20"] and lines[0].startswith("@HD")
    records = [l for l in lines if not l.startswith("@")]
    assert records == [bio.sam_record("read:%d:9" % i, _call(m)["sequence"], "5" * (m.r_en - m.r_st), m) for i, m in enumerate(good)]
    assert records[2].split("\t")[1] == "16" and records[2].split("\t")[9] == CONTIG[5:27]


def test_ctc_writer_arrays_orientation_and_order(tmp_path):
    from bonito_amd import io as bio
    maps = [_mapping(0, 20), _mapping(2, 23), _mapping(5, 27, strand=-1), _mapping(30, 52), _mapping(1, 22, strand=-1), _mapping(23, 44)]
    stream = [(_chunk(i), _call(m)) for i, m in enumerate(maps)]
    writer, _ = _run(stream, tmp_path, seed=11)
    chunks, refs, lens = (np.load(tmp_path / "ctc" / name) for name in ("chunks.npy", "references.npy", "reference_lengths.npy"))
    assert chunks.dtype == np.float16 and refs.dtype == np.uint8 and lens.dtype == np.uint16
    assert chunks.shape == (6, 16) and refs.shape == (6, 22) and lens.shape == (6,) and writer.shapes == (chunks.shape, refs.shape, lens.shape)
    np.random.seed(11)
    order = np.random.permutation(6)
    assert sorted(order.tolist()) != order.tolist()                      # the seed shuffles
    rows = [l.split("\t") for l in (tmp_path / "summary.tsv").read_text().strip().split("\n")]
    assert rows[0] == bio.summary_field_names + bio.alignment_field_names and len(rows) == 7
    for row, (k, i) in zip(rows[1:], enumerate(order)):
        m = maps[i]
        assert np.array_equal(chunks[k], _chunk(i).signal.astype(np.float16))
        label = "".join(" ACGT"[x] for x in refs[k, :lens[k]])
        # the label reads like the call: the reference under the alignment, reverse-complemented on the minus strand
        assert label == _call(m)["sequence"] and lens[k] == m.r_en - m.r_st and (refs[k, lens[k]:] == 0).all()
        assert row[1] == "read:%d:9" % i and row[11:14] == ["chr1", str(m.r_st), str(m.r_en)] and row[16] == ("+" if m.strand == 1 else "-")
    # the same seed, the same bytes; rna: the labels are reversed (back to signal order)
    _run(stream, tmp_path / "again", seed=11)
    for name in ("chunks.npy", "references.npy", "reference_lengths.npy"):
        assert (tmp_path / "ctc" / name).read_bytes() == (tmp_path / "again" / "ctc" / name).read_bytes()
    assert (tmp_path / "summary.tsv").read_bytes() == (tmp_path / "again" / "summary.tsv").read_bytes()
    _run(stream, tmp_path / "rna", seed=11, rna=True)
    refs_rna = np.load(tmp_path / "rna" / "ctc" / "references.npy")
    for k in range(6):
        assert refs_rna[k, :lens[k]].tolist() == refs[k, :lens[k]].tolist()[::-1]


def test_ctc_writer_drops_a_label_of_untypical_length(tmp_path):
    from bonito_amd import io as bio
    maps = [_mapping(i % 3, 20 + i % 5) for i in range(19)] + [_mapping(0, 45)]                  # one label twice as long as the others
    lens = np.array([m.r_en - m.r_st for m in maps])
    keep = bio.typical_indices(lens)
    assert keep.tolist() == list(range(19)) and abs(45 - lens.mean()) > 2.5 * lens.std()
    assert bio.typical_indices(np.array([5, 5, 5])).tolist() == []                                # strict on both sides
    writer, sam = _run([(_chunk(i), _call(m)) for i, m in enumerate(maps)], tmp_path)
    refs, lengths = np.load(tmp_path / "ctc" / "references.npy"), np.load(tmp_path / "ctc" / "reference_lengths.npy")
    assert refs.shape == (19, 45) and sorted(lengths.tolist()) == sorted(lens[:19].tolist())     # padded to the longest of ALL labels
    assert len((tmp_path / "summary.tsv").read_text().strip().split("\n")) == 20 and "read:19:9" not in (tmp_path / "summary.tsv").read_text()
    assert sam.count("\nread:") == 20                                                             # its SAM record had been written


def test_ctc_writer_without_an_accepted_chunk_writes_nothing(tmp_path, capsys):
    stream = [(_chunk(0), {"sequence": "ACGT" * 5, "qstring": "5" * 20, "mapping": None})]
    writer, sam = _run(stream, tmp_path)
    assert "> no suitable ctc data to write\n" in capsys.readouterr().err
    assert not (tmp_path / "ctc").exists() and not (tmp_path / "summary.tsv").exists() and writer.shapes is None
    assert dict(writer.rejected) == {"no_mapping": 1} and all(l.startswith("@") for l in sam.strip().split("\n"))


def test_ctc_output_directory(tmp_path):
    from bonito_amd import io as bio
    with open(tmp_path / "calls.sam", "w") as fh:
        assert bio.ctc_output_directory(fh.fileno()) == os.path.realpath(tmp_path)
    r, w = os.pipe()
    try:
        assert bio.ctc_output_directory(w) == "."
    finally:
        os.close(r)
        os.close(w)
    assert bio.ctc_output_directory(10 ** 6) == "."                      # no such descriptor


# ---- the parser ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra,words", [
    ([], "> a reference is needed to output ctc training data"),
    (["--reference", "ref.fa", "--devices", "0,1"], "--save-ctc runs on one device"),
    (["--reference", "ref.fa", "--device-ingest"], "--device-ingest cannot be combined"),
    (["--fasta"], "--fasta / --fastq cannot be combined"),
    (["--reference", "ref.fa", "--fastq"], "--fasta / --fastq cannot be combined"),
])
def test_save_ctc_refusals_come_before_any_model_is_loaded(extra, words, capsys):
    from bonito_amd.__main__ import main
    rc = main(["basecaller", "no/such/model", "no/such/reads", "--save-ctc"] + extra)
    err = capsys.readouterr().err
    assert rc == 1 and words in err and "loading model" not in err and "reading" not in err


def test_save_ctc_refuses_more_than_one_rank_and_turns_extend_ends_on(monkeypatch):
    from bonito_amd.cli import basecaller
    parse = basecaller.argparser().parse_args
    args = parse(["model", "reads", "--reference", "ref.fa"])
    assert (args.save_ctc, args.extend_ends, args.min_accuracy_save_ctc, args.ctc_output_dir) == (False, False, 0.99, None)
    assert basecaller.save_ctc_refusal(args) is None and args.extend_ends is False
    assert parse(["model", "reads", "--reference", "ref.fa", "--extend-ends"]).extend_ends is True
    args = parse(["model", "reads", "--reference", "ref.fa", "--save-ctc", "--min-accuracy-save-ctc", "0.95", "--ctc-output-dir", "out"])
    assert args.save_ctc and not args.extend_ends and (args.min_accuracy_save_ctc, args.ctc_output_dir) == (0.95, "out")
    assert basecaller.save_ctc_refusal(args) is None and args.extend_ends is True
    assert "one device" in basecaller.save_ctc_refusal(args, world=2)
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    assert basecaller.main(args) == 1

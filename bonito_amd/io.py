"""
Basecall output: FASTQ / FASTA / unaligned SAM text and ``summary.tsv`` -- the host-side formatting of
/root/reference bonito/io.py (encode_moves 57-70, write_fastq 97-105, sam_record 135-166, summary 169-226,
Writer 400-469) without pysam / mappy: aligned SAM text and the alignment columns of the summary come from the mappings of
bonito_amd/aligner.py (the device mapper, mappy's field names); BAM/CRAM need pysam and are out of scope.
SAM tags follow documentation/SAM.md:39-55: ``mv:B:c,<stride>,<moves...>``, ``qs:f`` (mean q-score),
``ns:i`` (samples incl. trimmed), ``ts:i`` (trimmed samples), ``RG:Z``.
"""
import csv
import os
import sys
from threading import Thread

import numpy as np

from bonito_amd.util import mean_qscore_from_qstring

__version__ = "0.1.0"

summary_field_names = ["filename", "read_id", "run_id", "channel", "mux", "start_time", "duration", "template_start",
                       "template_duration", "sequence_length_template", "mean_qscore_template"]
alignment_field_names = ["alignment_genome", "alignment_genome_start", "alignment_genome_end", "alignment_strand_start",
                         "alignment_strand_end", "alignment_direction", "alignment_length", "alignment_num_aligned",
                         "alignment_num_correct", "alignment_num_insertions", "alignment_num_deletions",
                         "alignment_num_substitutions", "alignment_mapq", "alignment_strand_coverage", "alignment_identity",
                         "alignment_accuracy"]


def mean_qscore(qstring):
    """`util.mean_qscore_from_qstring` through the library's helper: the Python records and the ones `bh_host_format_read` writes
    (crf/basecall.py `records_from_planes`) carry the same `qs:f` / summary values because they share the arithmetic."""
    try:
        from bonito_amd import _lib
        raw = qstring.encode("latin-1")
        return float(_lib.lib().bh_host_mean_qscore(raw, len(raw)))
    except OSError:                      # library not built: the numpy restatement (differs in the last bit at most)
        return float(mean_qscore_from_qstring(qstring))


def encode_moves(moves, stride, sep=","):
    """np.array([0,1,0,1,1]), 5 -> '5,0,1,0,1,1' (single-digit moves only)."""
    moves = np.asarray(moves)
    out = np.full(2 * moves.size, ord(sep), dtype=np.uint8)
    out[1::2] = moves.astype(np.uint8) + ord("0")
    return "%d%s" % (stride, out.tobytes().decode("ascii"))


def write_fasta(header, sequence, fd=sys.stdout):
    fd.write(">%s\n%s\n" % (header, sequence))


def write_fastq(header, sequence, qstring, fd=sys.stdout, tags=None, sep="\t"):
    fd.write("@%s%s\n" % (header, (" " + sep.join(tags)) if tags is not None else ""))
    fd.write("%s\n+\n%s\n" % (sequence, qstring))


def sam_header(groups, sep="\t", aligner=None):
    """With an aligner the header names its contigs (@SQ, what pysam writes from reference_names / reference_lengths in the
    reference's Writer, io.py:416-425) and the mapper (@PG ID:aligner)."""
    hd = sep.join(["@HD", "VN:1.5", "SO:unknown", "ob:%s" % __version__])
    pg = sep.join(["@PG", "ID:basecaller", "PN:bonito_amd", "VN:%s" % __version__, "CL:%s" % " ".join(sys.argv),
                   "DS:MI355X engine"])
    if aligner is None:
        return "\n".join([hd, pg, *groups]) + "\n"
    sq = [sep.join(["@SQ", "SN:%s" % name, "LN:%d" % len(aligner.seq(name))]) for name in aligner.seq_names]
    pg2 = sep.join(["@PG", "ID:aligner", "PN:bonito_amd", "VN:%s" % __version__, "DS:device mapper"])
    return "\n".join([hd, *sq, pg, pg2, *groups]) + "\n"


_COMPLEMENT = str.maketrans("ACGTacgt", "TGCAtgca")


def revcomp(sequence):
    return sequence[::-1].translate(_COMPLEMENT)


def sam_record(read_id, sequence, qstring, mapping=None, tags=None, sep="\t"):
    if mapping:
        # the reference's record (bonito/io.py:139-157) as it stands: on the minus strand the sequence is reverse-complemented and the
        # soft-clips swap ends, but the q-string is written as basecalled, NOT reversed
        plus = mapping.strand == +1
        softclip = ["%sS" % mapping.q_st if mapping.q_st else "", mapping.cigar_str,
                    "%sS" % (len(sequence) - mapping.q_en) if len(sequence) - mapping.q_en else ""]
        record = [read_id, 0 if plus else 16, mapping.ctg, mapping.r_st + 1, mapping.mapq, "".join(softclip if plus else softclip[::-1]),
                  "*", 0, 0, sequence if plus else revcomp(sequence), qstring, "NM:i:%s" % mapping.NM, "MD:Z:%s" % mapping.MD]
    else:
        record = [read_id, 4, "*", 0, 0, "*", "*", 0, 0, sequence, qstring, "NM:i:0"]
    if tags is not None:
        record.extend(tags)
    return sep.join(map(str, record))


def read_tags(read, res, mean_q):
    tags = ["RG:Z:%s" % (read.run_id or "unknown"), "qs:f:%0.2f" % mean_q, "ns:i:%d" % read.num_samples,
            "ts:i:%d" % read.trimmed_samples]
    if res.get("moves") is not None and len(res["moves"]):
        tags.append("mv:B:c,%s" % encode_moves(res["moves"], res["stride"]))
    return tags


def summary_row(read, seqlen, qscore, alignment=False):
    """alignment: False = no alignment columns; a mapping = the reference's 16 columns (bonito/io.py:229-251); None = its row for
    an unmapped read (io.py:253-256)."""
    fields = [read.filename, read.read_id, read.run_id, read.channel, read.mux, read.start, read.duration,
              read.template_start, read.template_duration, seqlen, qscore]
    if alignment:
        ins = sum(count for count, op in alignment.cigar if op == 1)
        dels = sum(count for count, op in alignment.cigar if op == 2)
        subs = alignment.NM - ins - dels
        length = alignment.blen
        matches = length - ins - dels
        correct = alignment.mlen
        plus = alignment.strand == +1
        fields.extend([alignment.ctg, alignment.r_st, alignment.r_en, alignment.q_st if plus else seqlen - alignment.q_en,
                       alignment.q_en if plus else seqlen - alignment.q_st, "+" if plus else "-", length, matches, correct, ins, dels,
                       subs, alignment.mapq, (alignment.q_en - alignment.q_st) / seqlen, correct / matches, correct / length])
    elif alignment is None:
        fields.extend(["*", -1, -1, -1, -1, "*", 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0])
    return fields


def signal_samples(read):
    """Post-trim samples of a read: what the reference logs as ``len(read.signal)`` (io.py:437-440) and the CLI divides
    by the wall time for its `samples per second` line (cli/basecaller.py:156-164)."""
    sig = getattr(read, "signal", None)
    if sig is not None:
        return len(sig)
    n = getattr(read, "signal_len", None)                 # RawRead: filled in by the device ingest
    return int(n) if n is not None else int(read.num_samples) - int(getattr(read, "trimmed_samples", 0))


def format_record(read, res, mode, min_qscore=0.0):
    """One basecalled read -> (text to write or None, summary row or None, (read_id, post-trim samples)).

    The single place that turns a (read, result) pair into output bytes: the in-process `Writer` and the per-rank workers of
    the multi-GPU path (bonito_amd/parallel.py) both call it, so N-rank output is byte-identical to 1-rank output by
    construction. The log entry is produced for EVERY read, before the q-score / empty-sequence filters, like the reference
    (io.py:437-442)."""
    seq, qstring = res["sequence"], res.get("qstring", "*")
    # Reference semantics (bonito/io.py:431-433, util.py:114-121): the mean q-score is ALWAYS computed from the q-string - 9.0 for the
    # "*" sentinel as for a real one-base read with Q9 (whose q-string IS "*"), 0.0 for an empty one. Only the formatting differs: the
    # sentinel / an empty q-string beside a sequence mean "no qualities" ('!' per base in FASTQ, where the reference would write a
    # malformed record; '*' in SAM). A decoded "*" beside ONE base is a quality and is written unchanged (advisor finding, round 4).
    no_quals = len(qstring) == 0 or (qstring == "*" and len(seq) != 1)
    mean_q = mean_qscore(qstring) if len(qstring) else 0.0
    log = (read.read_id, signal_samples(read))
    if mean_q < min_qscore or not len(seq):
        return None, None, log
    if mode == "fasta":
        text = ">%s\n%s\n" % (read.read_id, seq)
    elif mode == "fastq":
        tags = read_tags(read, res, mean_q)
        text = "@%s %s\n%s\n+\n%s\n" % (read.read_id, "\t".join(tags), seq, "!" * len(seq) if no_quals else qstring)
    else:
        text = sam_record(read.read_id, seq, "*" if no_quals else qstring, res.get("mapping"), tags=read_tags(read, res, mean_q)) + "\n"
    # a result that went through aligner.align_map carries "mapping" (None = unmapped): the summary then has the alignment columns
    return text, summary_row(read, len(seq), mean_q, alignment=res["mapping"] if "mapping" in res else False), log


class Writer(Thread):
    """Consumes the basecall iterator (this drives the whole pipeline) and writes records to `fd`.

    `iterator` yields (read, result) pairs, or -- `preformatted=True`, the multi-GPU merge of bonito_amd/parallel.py --
    the (text, summary_row, log) triples `format_record` made of them on the rank that basecalled the read. A pre-formatted
    text may be `bytes` / a memoryview and a row the rendered TSV line as `bytes` (the packed blocks of parallel.ordered_records, the
    library's record text taken as it is): they go to the binary layer of `fd` without a str round trip."""

    def __init__(self, mode, iterator, fd=sys.stdout, min_qscore=0.0, summary_path=None, groups=(), preformatted=False, aligner=None):
        super().__init__()
        self.aligner = aligner   # its contigs go to the SAM header, the alignment columns to the summary's
        assert mode in ("fastq", "fasta", "sam")
        self.mode, self.iterator, self.fd = mode, iterator, fd
        self.min_qscore, self.summary_path, self.groups = min_qscore, summary_path, groups
        self.preformatted = preformatted
        self.log = []            # (read_id, post-trim samples) of every basecalled read: feeds the samples/s report
        self.error = None

    def run(self):
        try:
            summary = open(self.summary_path, "w", newline="") if self.summary_path else None
            tsv = csv.writer(summary, delimiter="\t") if summary else None
            if tsv:
                tsv.writerow(summary_field_names + (alignment_field_names if self.aligner is not None else []))
            if self.mode == "sam":
                self.fd.write(sam_header(self.groups, aligner=self.aligner))
            raw = getattr(self.fd, "buffer", None)          # the binary layer under a text file (sys.stdout, open(..., "w")); None for StringIO
            dirty = self.mode == "sam"                      # text written through the str layer and not yet flushed
            for item in self.iterator:
                text, row, log = item if self.preformatted else format_record(item[0], item[1], self.mode, self.min_qscore)
                self.log.append(log)
                if text is None:
                    continue
                if isinstance(text, str):
                    self.fd.write(text)
                    dirty = True
                elif raw is not None:
                    if dirty:
                        self.fd.flush()
                        dirty = False
                    raw.write(text)
                else:
                    self.fd.write(bytes(text).decode("utf-8"))
                if tsv:
                    if isinstance(row, (bytes, bytearray, memoryview)):
                        summary.write(bytes(row).decode("utf-8"))          # rendered by the csv module on the producing rank
                    else:
                        tsv.writerow(row)
            if raw is not None:
                raw.flush()
            self.fd.flush()
            if summary:
                summary.close()
        except BaseException as exc:       # surfaced by the caller after join()
            self.error = exc


class CSVLogger:
    """Appends dict rows to a CSV file (losses_N.csv, training.csv of a training run; the reference's bonito/io.py CSVLogger). The
    first row ever written fixes the columns and writes the header; a file that exists already keeps its header, and its columns
    choose what later rows contribute ('-' where a row lacks one)."""

    def __init__(self, filename, sep=","):
        self.filename = str(filename)
        self.columns = None
        if os.path.exists(self.filename):
            with open(self.filename, newline="") as fh:
                self.columns = csv.DictReader(fh, delimiter=sep).fieldnames
        self.fh = open(self.filename, "a", newline="")
        self.writer = csv.writer(self.fh, delimiter=sep)
        self.unflushed = 0

    def set_columns(self, columns):
        if self.columns:
            raise ValueError("CSVLogger: the columns of %s are set already" % self.filename)
        self.columns = list(columns)
        self.writer.writerow(self.columns)

    def append(self, row):
        if self.columns is None:
            self.set_columns(row.keys())
        self.writer.writerow([row.get(k, "-") for k in self.columns])
        self.unflushed += 1
        if self.unflushed > 100:
            self.unflushed = 0
            self.fh.flush()

    def close(self):
        self.fh.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class RejectCounter(dict):
    """Counts the reasons for which chunks are rejected (bonito/io.py:505-510)."""

    def __call__(self, reject_condition, condition_name):
        if reject_condition:
            self[condition_name] = self.get(condition_name, 0) + 1
        return reject_condition


def typical_indices(x, n=2.5):
    """Indices of the values strictly within n standard deviations of the mean (bonito/io.py:29-32)."""
    mu, sd = np.mean(x), np.std(x)
    idx, = np.where((mu - n * sd < x) & (x < mu + n * sd))
    return idx


def ctc_output_directory(fd=1):
    """Where the reference's CTCWriter puts its arrays (bonito/io.py:605): the directory of the regular file behind stdout, '.' when
    stdout is a terminal, a pipe or anything else without a directory of its own."""
    import os
    import stat
    try:
        if os.isatty(fd) or not stat.S_ISREG(os.fstat(fd).st_mode):
            return "."
        path = os.path.realpath("/dev/fd/%d" % fd)
    except OSError:
        return "."
    directory = os.path.dirname(path)
    return directory if directory and not path.startswith("/proc/") and os.path.isdir(directory) else "."


class CTCWriter(Thread):
    """``basecaller --save-ctc`` (bonito/io.py:513-616): consumes (chunk, result) pairs whose results went through ``align_map``, keeps
    the chunks whose call maps with at least `min_accuracy` and `min_coverage` to an N-free stretch of the reference, writes their SAM
    records to `fd` as they come and, at the end, ``chunks.npy`` (float16 [n, chunksize]), ``references.npy`` (uint8, A C G T = 1 2 3 4,
    zero-padded) and ``reference_lengths.npy`` (uint16) to `output_directory`, rows of typical length only and shuffled with numpy's
    global generator; the summary holds the same rows in the same order. The label of a chunk is the reference under its alignment,
    which is why the mappings must have their ends extended (``Aligner(extend_ends=True)``)."""

    def __init__(self, mode, iterator, aligner, fd=sys.stdout, min_coverage=0.90, min_accuracy=0.99, groups=(), min_qscore=0.0,
                 rna=False, summary_path="summary.tsv", output_directory="."):
        super().__init__()
        assert mode == "sam"
        self.mode, self.iterator, self.aligner, self.fd = mode, iterator, aligner, fd
        self.min_coverage, self.min_accuracy, self.min_qscore, self.rna = min_coverage, min_accuracy, min_qscore or 0.0, rna
        self.groups, self.summary_path, self.output_directory = groups, summary_path, output_directory
        self.log = []
        self.rejected = RejectCounter()
        self.shapes = None           # the shapes of the three arrays once they are written
        self.error = None

    def run(self):
        try:
            self._run()
        except BaseException as exc:       # surfaced by the caller after join()
            self.error = exc

    def _run(self):
        import os
        chunks, targets, lengths, rows = [], [], [], []
        reject = self.rejected
        self.fd.write(sam_header(self.groups, aligner=self.aligner))
        for read, res in self.iterator:
            seq, qstring = res["sequence"], res["qstring"]
            mean_q = res["mean_qscore"] if "mean_qscore" in res else (mean_qscore(qstring) if len(qstring) else 0.0)
            mapping = res.get("mapping")
            self.log.append((read.read_id, len(read.signal)))
            if reject(mean_q < self.min_qscore, "low_qscore"):
                continue
            if reject(len(seq) == 0, "zerolen_sequence"):
                continue
            if reject(not mapping, "no_mapping"):
                continue
            cov = (mapping.q_en - mapping.q_st) / len(seq)
            acc = mapping.mlen / mapping.blen
            refseq = self.aligner.seq(mapping.ctg, mapping.r_st, mapping.r_en)
            if reject(acc < self.min_accuracy, "low_accuracy%.2f" % self.min_accuracy):
                continue
            if reject(cov < self.min_coverage, "low_coverage%.2f" % self.min_coverage):
                continue
            if reject(bool(set(refseq) - set("ACGT")), "N_in_sequence"):      # N, and any other letter that is no label
                continue
            self.fd.write(sam_record(read.read_id, seq, qstring, mapping) + "\n")
            rows.append(summary_row(read, len(seq), mean_q, alignment=mapping))
            if mapping.strand == -1:
                refseq = revcomp(refseq)
            target = ["ACGT".index(base) + 1 for base in refseq]
            targets.append(target[::-1] if self.rna else target)      # an RNA call is already reversed: back to signal order
            chunks.append(read.signal)
            lengths.append(len(target))
        self.fd.flush()
        if len(chunks) == 0:
            sys.stderr.write("> no suitable ctc data to write\n")
            return
        chunks = np.array(chunks, dtype=np.float16)
        targets_ = np.zeros((chunks.shape[0], max(lengths)), dtype=np.uint8)
        for idx, target in enumerate(targets):
            targets_[idx, :len(target)] = target
        lengths = np.array(lengths, dtype=np.uint16)
        indices = np.random.permutation(typical_indices(lengths))
        chunks, targets_, lengths = chunks[indices], targets_[indices], lengths[indices]
        if self.summary_path:
            with open(self.summary_path, "w", newline="") as summary:
                tsv = csv.writer(summary, delimiter="\t")
                tsv.writerow(summary_field_names + alignment_field_names)
                for idx in indices:
                    tsv.writerow(rows[idx])
        os.makedirs(self.output_directory, exist_ok=True)
        np.save(os.path.join(self.output_directory, "chunks.npy"), chunks)
        np.save(os.path.join(self.output_directory, "references.npy"), targets_)
        np.save(os.path.join(self.output_directory, "reference_lengths.npy"), lengths)
        self.shapes = (chunks.shape, targets_.shape, lengths.shape)
        sys.stderr.write("> Chunks rejected from training data:\n")
        for condition_name, count in reject.items():
            sys.stderr.write(" - %s: %d\n" % (condition_name, count))
        sys.stderr.write("> written ctc training data to %s\n" % self.output_directory)
        sys.stderr.write("  - chunks.npy with shape (%s)\n" % ",".join(map(str, chunks.shape)))
        sys.stderr.write("  - references.npy with shape (%s)\n" % ",".join(map(str, targets_.shape)))
        sys.stderr.write("  - reference_lengths.npy shape (%s)\n" % ",".join(map(str, lengths.shape)))

    def stop(self):
        self.join()

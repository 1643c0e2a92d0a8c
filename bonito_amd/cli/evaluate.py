"""
``python -m bonito_amd evaluate``: score a checkpoint on bonito's labelled chunk data (chunks.npy, references.npy,
reference_lengths.npy) with the HIP engine -- the arguments of the reference's bonito/cli/evaluate.py:140-155.

Per batch: engine forward, ``decode_batch`` (posterior decoding) and ``loss(..., reduction='none')``, i.e.
-ln P(reference | scores) / reference length per chunk from the sequence-likelihood kernel. A bonito.ctc model (no ``decode_batch``)
is decoded by prefix beam search of width 5 and scored by the CTC loss kernel (the 'loss' entry of its dict). After the calling loop every called
sequence is aligned against its reference in ONE ``align.sw_align`` call (Smith-Waterman on the device, the reference's parasail
arguments; evaluate.py:37-67). Printed: the reference's block (accuracy, sub / ins / del rates, lengths and clips; evaluate.py:117-129)
plus mean and median loss. With ``--output_dir``: seqs.fasta, refs.fasta and summ.txt (per-chunk TSV: loss and the AlignResult columns).
"""
import os
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser
from pathlib import Path

import numpy as np
import torch

from bonito_amd.data import load_numpy_datasets
from bonito_amd.util import decode_ref, init, load_model

SUMM_COLUMNS = ("accuracy", "num_correct", "num_mismatches", "num_insertions", "num_deletions", "ref_len", "seq_len",
                "align_ref_start", "align_ref_end", "align_seq_start", "align_seq_end")


def load_chunks(directory, dataset="valid", chunks=512):
    """The (chunks, references, lengths) the reference's evaluate would iterate over, in order (bonito/data.py:99-119 through
    cli/evaluate.py:87-95): ``valid`` = the first `chunks` of the validation/ sub-directory when one exists, otherwise the tail
    split (the last `chunks`) of the first 100 * chunks training chunks; ``train`` = the training side of that split for
    limit = chunks (the reference shuffles it; the order here is the file's)."""
    directory = str(directory)
    limit = chunks * 100 if dataset == "valid" else chunks
    has_valid = os.path.exists(os.path.join(directory, "validation"))
    if dataset == "valid" and has_valid:
        return load_numpy_datasets(limit=chunks, directory=os.path.join(directory, "validation"))
    data = load_numpy_datasets(limit=limit, directory=directory)
    if has_valid:
        return data
    split = max(0, len(data[0]) - chunks)
    return tuple(x[split:] if dataset == "valid" else x[:split] for x in data)


def report_lines(table, seq_len, ref_len, losses):
    """The printed block from arrays: `table` int [n, 10] in align.COLUMNS order, lengths and losses per chunk. The three rates
    divide by num_correct as the reference's do (evaluate.py:120-122), so they are averaged over the chunks with num_correct > 0
    and the number of chunks left out is printed; accuracy and the clips average over every chunk (an unaligned chunk: accuracy 0,
    its whole length as right clip)."""
    table = np.asarray(table, np.int64).reshape(-1, 10)
    seq_len, ref_len, losses = np.asarray(seq_len, np.int64), np.asarray(ref_len, np.int64), np.asarray(losses, np.float64)
    n = len(table)
    correct, mism, ins, dele = (table[:, c] for c in (1, 2, 3, 4))
    ref_start, ref_end, seq_start, seq_end = (table[:, c] for c in (5, 6, 7, 8))
    total = correct + mism + ins + dele
    acc = np.divide(correct, total, out=np.zeros(n), where=total > 0)
    ok = correct > 0

    def mean(x):
        return float(np.mean(x)) if len(x) else 0.0

    def rate(x):
        return mean(x[ok] / correct[ok])

    return [
        "* num_chunks      %d" % n,
        "* loss mean       %.4f" % (losses.mean() if len(losses) else float("nan")),
        "* loss median     %.4f" % (np.median(losses) if len(losses) else float("nan")),
        "* accuracy        %.2f%%" % (100 * mean(acc)),
        "* sub-rate        %.2f%%" % (100 * rate(mism)),
        "* ins-rate        %.2f%%" % (100 * rate(ins)),
        "* del-rate        %.2f%%" % (100 * rate(dele)),
        "* rates left out  %d chunks with num_correct = 0" % int(n - ok.sum()),
        "* seq_len         %.1f" % mean(seq_len),
        "* seq_lclip       %.1f" % mean(seq_start),
        "* seq_rclip       %.1f" % mean(seq_len - seq_end - 1),
        "* ref_len         %.1f" % mean(ref_len),
        "* ref_lclip       %.1f" % mean(ref_start),
        "* ref_rclip       %.1f" % mean(ref_len - ref_end - 1),
    ]


def summ_lines(table, seq_len, ref_len, losses):
    """summ.txt: a header and one tab-separated row per chunk, `loss` and then the AlignResult columns of the reference's table."""
    table = np.asarray(table, np.int64).reshape(-1, 10)
    lines = ["\tloss\t" + "\t".join(SUMM_COLUMNS) + "\n"]
    for i, (row, s, r, l) in enumerate(zip(table, seq_len, ref_len, losses)):
        total = int(row[1:5].sum())
        acc = row[1] / total if total else 0.0
        lines.append("%d\t%.6f\t%.6f\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n"
                     % (i, l, acc, row[1], row[2], row[3], row[4], r, s, row[5], row[6], row[7], row[8]))
    return lines


def decode_batch(model, scores):
    """The called sequence of every chunk: the model's own ``decode_batch`` (CRF family), else - bonito.ctc - the prefix beam search of
    ctc/basecall.py:decode_grouped at the reference's beam width 5 (evaluate.py:110) over the [T, N, C] log-probabilities."""
    if hasattr(model, "decode_batch"):
        return model.decode_batch(scores)
    from bonito_amd.ctc.basecall import decode_grouped
    lps = scores.permute(1, 0, 2).to(torch.float32)
    return [v["sequence"] for _, v in decode_grouped(model, ((i, {"scores": lp}) for i, lp in enumerate(lps)), beamsize=5)]


def main(args):
    init(args.seed, args.device)
    if args.directory is None:
        raise SystemExit("evaluate: --directory (chunks.npy, references.npy, reference_lengths.npy) is required")
    print("* loading model from: %s/weights_%s.tar" % (args.model_directory, args.weights))
    model = load_model(args.model_directory, args.device, weights=args.weights, batchsize=args.batchsize)
    std = model.config.get("standardisation", {}) if args.standardise else {}
    mean, stdev = std.get("mean", 0.0), std.get("stdev", 1.0)
    print("* * applying standardisation params: mean=%s, stdev=%s" % (mean, stdev))

    print("* loading data")
    chunks, targets, lengths = load_chunks(args.directory, args.dataset, args.chunks)
    print("* calling")
    seqs, losses = [], []
    for lo in range(0, len(lengths), args.batchsize):
        x = (torch.from_numpy(np.asarray(chunks[lo:lo + args.batchsize], dtype=np.float32)) - mean) / stdev
        x = x.unsqueeze(1).to(torch.float16).to(args.device)
        t = torch.from_numpy(np.asarray(targets[lo:lo + args.batchsize]).astype(np.int32))
        n = torch.from_numpy(np.asarray(lengths[lo:lo + args.batchsize]).astype(np.int32))
        t = t[:, :max(int(n.max()), 1)]
        scores = model(x)
        seqs.extend(decode_batch(model, scores))
        loss = model.loss(scores, t, n, reduction="none")
        losses.append((loss["loss"] if isinstance(loss, dict) else loss).cpu().numpy())
    losses = np.concatenate(losses) if losses else np.zeros(0, np.float32)
    refs = [decode_ref(t[:n], model.alphabet) for t, n in zip(targets, lengths)]
    print("* aligning")
    from bonito_amd.align import sw_align
    aligned = sw_align(seqs, refs)
    print("\n".join([""] + report_lines(aligned.table, aligned.seq_len, aligned.ref_len, losses) + [""]))
    if args.output_dir:
        args.output_dir.mkdir(exist_ok=True, parents=True)
        with (args.output_dir / "seqs.fasta").open("w") as fh:
            fh.write("".join(">chunk_%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
        with (args.output_dir / "refs.fasta").open("w") as fh:
            fh.write("".join(">chunk_%d\n%s\n" % (i, s) for i, s in enumerate(refs)))
        with (args.output_dir / "summ.txt").open("w") as fh:
            fh.write("".join(summ_lines(aligned.table, aligned.seq_len, aligned.ref_len, losses)))
    return 0


def argparser():
    parser = ArgumentParser(
        formatter_class=ArgumentDefaultsHelpFormatter,
        add_help=False,
        description="Loss and alignment accuracy of labelled chunks on the HIP engine (Smith-Waterman on the device with the "
                    "reference's parasail arguments); --output_dir receives seqs.fasta, refs.fasta and summ.txt.",
    )
    parser.add_argument("model_directory")
    parser.add_argument("--output_dir", type=Path)
    parser.add_argument("--directory", type=Path)
    parser.add_argument("--dataset", choices=["train", "valid"], default="valid")
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--seed", default=9, type=int)
    parser.add_argument("--weights", default=0, type=None)
    parser.add_argument("--chunks", default=512, type=int)
    parser.add_argument("--batchsize", default=256, type=int)
    parser.add_argument("--standardise", action="store_true", default=False)
    return parser

"""
``python -m bonito_amd evaluate``: score a checkpoint on bonito's labelled chunk data (chunks.npy, references.npy,
reference_lengths.npy) with the HIP engine -- the arguments of the reference's bonito/cli/evaluate.py:140-155.

Per batch: engine forward, ``decode_batch`` (posterior decoding) and ``loss(..., reduction='none')``, i.e.
-ln P(reference | scores) / reference length per chunk from the sequence-likelihood kernel. Printed: num_chunks, mean and median
loss, mean called / reference lengths. With ``--output_dir``: seqs.fasta, refs.fasta and summ.txt (per-chunk TSV of loss and lengths).

Alignment accuracy is NOT reported: the reference computes it with parasail (sw_trace_striped_32, evaluate.py:37-67), which this
engine neither ships nor re-implements. seqs.fasta / refs.fasta are what an external aligner needs.
"""
import os
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser
from pathlib import Path

import numpy as np
import torch

from bonito_amd.util import init, load_model


def load_numpy_datasets(limit=None, directory=None):
    """chunks, references, reference_lengths of a directory (reference bonito/data.py:122-144)."""
    chunks = np.load(os.path.join(directory, "chunks.npy"), mmap_mode="r")
    targets = np.load(os.path.join(directory, "references.npy"), mmap_mode="r")
    lengths = np.load(os.path.join(directory, "reference_lengths.npy"), mmap_mode="r")
    indices = os.path.join(directory, "indices.npy")
    if os.path.exists(indices):
        idx = np.load(indices, mmap_mode="r")
        idx = idx[idx < lengths.shape[0]]
        if limit:
            idx = idx[:limit]
        return chunks[idx, :], targets[idx, :], lengths[idx]
    if limit:
        chunks, targets, lengths = chunks[:limit], targets[:limit], lengths[:limit]
    return np.array(chunks), np.array(targets), np.array(lengths)


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


def decode_ref(encoded, labels):
    """Integer-encoded reference -> string (reference util.py decode_ref)."""
    return "".join(labels[int(e)] for e in encoded if e)


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
        seqs.extend(model.decode_batch(scores))
        losses.append(model.loss(scores, t, n, reduction="none").cpu().numpy())
    losses = np.concatenate(losses) if losses else np.zeros(0, np.float32)
    refs = [decode_ref(t[:n], model.alphabet) for t, n in zip(targets, lengths)]
    seq_len = np.array([len(s) for s in seqs])
    ref_len = np.array([len(r) for r in refs])
    print("\n".join([
        "",
        "* num_chunks      %d" % len(refs),
        "* loss mean       %.4f" % (losses.mean() if len(losses) else float("nan")),
        "* loss median     %.4f" % (np.median(losses) if len(losses) else float("nan")),
        "* seq_len         %.1f" % (seq_len.mean() if len(seq_len) else 0.0),
        "* ref_len         %.1f" % (ref_len.mean() if len(ref_len) else 0.0),
        "* accuracy        not computed (no aligner in this engine; align seqs.fasta against refs.fasta)",
        "",
    ]))
    if args.output_dir:
        args.output_dir.mkdir(exist_ok=True, parents=True)
        with (args.output_dir / "seqs.fasta").open("w") as fh:
            fh.write("".join(">chunk_%d\n%s\n" % (i, s) for i, s in enumerate(seqs)))
        with (args.output_dir / "refs.fasta").open("w") as fh:
            fh.write("".join(">chunk_%d\n%s\n" % (i, s) for i, s in enumerate(refs)))
        with (args.output_dir / "summ.txt").open("w") as fh:
            fh.write("\tloss\tref_len\tseq_len\n")
            fh.write("".join("%d\t%.6f\t%d\t%d\n" % (i, l, r, s) for i, (l, r, s) in enumerate(zip(losses, ref_len, seq_len))))
    return 0


def argparser():
    parser = ArgumentParser(
        formatter_class=ArgumentDefaultsHelpFormatter,
        add_help=False,
        description="Loss and called sequences of labelled chunks on the HIP engine. Alignment accuracy is not computed "
                    "(the reference uses parasail); seqs.fasta / refs.fasta in --output_dir feed an external aligner.",
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

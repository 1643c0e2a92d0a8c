#!/usr/bin/env python3
"""
Generate tests/golden/crf_ctc_loss.npz by EXECUTING THE REFERENCE's CTC_CRF.prepare_ctc_scores / ctc_loss /
ctc_viterbi_alignments (bonito/crf/model.py:110-143) on PyTorch-CPU. Run where the reference checkout is available:

    python tests/golden/make_golden_seqdist.py

The reference class is imported exactly as make_golden.ref_crf_model() does (koi replaced by a torch stub). The two further
koi.ctc names these methods call are bound to the torch restatement in tests/seqdist_ref.py [EXT: koi is closed source]:
  * logZ_cu(stay_scores, move_scores, n): alpha_0 = [0, -inf, ..]; alpha_{t+1}[j] = logaddexp(alpha_t[j] + stay_t[j],
    alpha_t[j-1] + move_t[j-1]); result alpha_T[n - 1];
  * viterbi_alignments(stay_scores, move_scores, n): the same scan with max and a traceback, in this project's compact form
    (position after every step, ties stay) - what koi returns is unknown and the reference never calls it.
Everything else (normalise, the k-mer index arithmetic and the two gathers, `- logz / target_lengths`, loss_clip, reduction)
is the reference's own code, executed in fp32 as SeqdistModel.loss does (crf/model.py:204-207).

Scores lie on a grid of 1/8 within +-5 (exact in fp16; partial sums of these short chunks are exact in fp32 and fp64 alike, so
the Max-scan alignments do not depend on the accumulation precision). Cases: state_len 1..5 in the koi layout (fixed blank 2.0,
stored as the engine's [N, T, 4S]; the reference sees the expanded [T, N, 5S]) and state_len 1..3 with a learned, non-constant
stay column (stored as [T, N, 5S]). Target lengths run from state_len to beyond T (no alignment: logz = -inf, loss = +inf).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden  # noqa: E402
import seqdist_ref  # noqa: E402

CLIP = 1.5
SHAPES = {1: (40, 4), 2: (48, 4), 3: (48, 4), 4: (36, 4), 5: (20, 4)}      # state_len -> (T, N)


def main():
    cm = make_golden.ref_crf_model()
    cm.logZ_cu = seqdist_ref.torch_logz_cu
    cm.viterbi_alignments = seqdist_ref.torch_viterbi_alignments
    gen = torch.Generator().manual_seed(27)
    out = {"cases": [], "loss_clip": np.float32(CLIP)}
    for layout in ("koi", "5s"):
        for sl in (1, 2, 3, 4, 5) if layout == "koi" else (1, 2, 3):
            T, N = SHAPES[sl]
            S = 4 ** sl
            sd = cm.CTC_CRF(sl, ["N", "A", "C", "G", "T"])
            x4 = torch.round((torch.randn(T, N, 4 * S, generator=gen) * 2.0).clamp(-5, 5) * 8) / 8
            if layout == "koi":
                x5 = torch.nn.functional.pad(x4.view(T, N, S, 4), (1, 0), value=2.0).view(T, N, 5 * S)      # nn.py:291-297
            else:
                stay = torch.round((torch.randn(T, N, S, 1, generator=gen) + 1.0).clamp(-5, 5) * 8) / 8
                x5 = torch.cat([stay, x4.view(T, N, S, 4)], dim=-1).view(T, N, 5 * S)
            lengths = torch.tensor([sl, max(sl, T // 3), (4 * T) // 5, T + sl + 2][:N])
            Lmax = int(lengths.max())
            targets = torch.randint(1, 5, (N, Lmax), generator=gen)
            targets = torch.where(torch.arange(Lmax)[None, :] < lengths[:, None], targets, torch.zeros_like(targets))
            name = "sl%d_%s" % (sl, layout)
            out["cases"].append(name)
            f32 = x5.float()
            out[name + "/scores"] = (x4.permute(1, 0, 2).contiguous() if layout == "koi" else x5).half().numpy()
            out[name + "/blank"] = np.float32(2.0 if layout == "koi" else np.nan)
            out[name + "/targets"] = targets.numpy().astype(np.int8)
            out[name + "/lengths"] = lengths.numpy().astype(np.int32)
            for norm in (True, False):
                for red in ("none", "mean"):
                    v = sd.ctc_loss(f32, targets, lengths, reduction=red, normalise_scores=norm)
                    out["%s/loss_%s_%s" % (name, "norm" if norm else "raw", red)] = v.numpy()
            out[name + "/loss_clip_none"] = sd.ctc_loss(f32, targets, lengths, loss_clip=CLIP, reduction="none").numpy()
            out[name + "/loss_clip_mean"] = sd.ctc_loss(f32, targets, lengths, loss_clip=CLIP, reduction="mean").numpy()
            out[name + "/align"] = sd.ctc_viterbi_alignments(f32, targets, lengths).numpy()
            if sl == 2:                                       # the small case whose gathered edges are kept
                stay_s, move_s = sd.prepare_ctc_scores(f32, targets)
                out[name + "/stay_scores"] = stay_s.numpy()
                out[name + "/move_scores"] = move_s.numpy()
            print("%-8s T=%d N=%d lengths %s  loss(norm) %s" % (name, T, N, lengths.tolist(),
                                                               np.round(out[name + "/loss_norm_none"], 4).tolist()))
    out["cases"] = np.array(out["cases"])
    path = os.path.join(HERE, "crf_ctc_loss.npz")
    np.savez_compressed(path, **out)
    print("%s: %d KiB" % (path, os.path.getsize(path) // 1024))


if __name__ == "__main__":
    main()

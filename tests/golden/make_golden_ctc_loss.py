#!/usr/bin/env python3
"""
Generate tests/golden/ctc_loss.npz by EXECUTING THE REFERENCE's Model.ctc_label_smoothing_loss (bonito/ctc/model.py:48-54) on
PyTorch-CPU, on fp32 and on fp16 log_probs. Run where the reference checkout is available:

    python tests/golden/make_golden_ctc_loss.py

The reference module is imported as make_golden.ref_ctc() does. Next to the reference's dict every case records torch's fp64
per-chunk ctc_loss (reduction='none') and its gradient with respect to the LOGITS (log_softmax in front, zero_infinity=True so that the
chunks without an alignment carry zeros instead of NaN), and - where every chunk has an alignment - the fp64 gradient of the
reference's total_loss formula with respect to the logits.

Cases (seeded logits, log_probs = log_softmax(logits)):
  t48_c5    T = 48, C = 5, lengths 0, 1, 5, 16, a 24-long homopolymer (needs 47 steps), 40
  t48_inf   T = 48, C = 5, lengths 47, 48, 49, 30: the first three have no alignment (+inf)
  t40_c2    T = 40, C = 2 (one label: every target is a homopolymer), lengths 0, 1, 5, 20
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden  # noqa: E402

CASES = {"t48_c5": (48, 5, [0, 1, 5, 16, 24, 40]), "t48_inf": (48, 5, [47, 48, 49, 30]), "t40_c2": (40, 2, [0, 1, 5, 20])}


def main():
    cm = make_golden.ref_ctc()
    ref_loss = cm.Model.ctc_label_smoothing_loss
    gen = torch.Generator().manual_seed(31)
    out = {"cases": np.array(sorted(CASES))}
    for name in sorted(CASES):
        T, C, lens = CASES[name]
        N, Lmax = len(lens), max(lens)
        logits = (torch.randn(T, N, C, generator=gen) * 2.0).float()
        lengths = torch.tensor(lens)
        targets = torch.randint(1, C, (N, Lmax), generator=gen)
        if name == "t48_c5":
            targets[4, :] = 3                                               # the homopolymer row
        targets = torch.where(torch.arange(Lmax)[None, :] < lengths[:, None], targets, torch.zeros_like(targets))
        lp32 = F.log_softmax(logits, dim=-1)
        for tag, lp in (("ref32", lp32), ("ref16", lp32.half())):
            d = ref_loss(None, lp, targets, lengths)
            out["%s/%s" % (name, tag)] = np.array([float(d["total_loss"]), float(d["loss"]), float(d["label_smooth_loss"])], np.float64)
        x = logits.double().requires_grad_(True)
        lp64 = F.log_softmax(x, dim=-1)
        per = F.ctc_loss(lp64, targets, torch.full((N,), T, dtype=torch.int64), lengths, reduction="none", zero_infinity=True)
        true = F.ctc_loss(lp64.detach(), targets, torch.full((N,), T, dtype=torch.int64), lengths, reduction="none")
        per.sum().backward()
        out[name + "/logits"] = logits.numpy()
        out[name + "/targets"] = targets.numpy().astype(np.int8)
        out[name + "/lengths"] = lengths.numpy().astype(np.int32)
        out[name + "/nll64"] = true.numpy()
        out[name + "/grad_logits64"] = x.grad.numpy().copy()
        if bool(torch.isfinite(true).all()):
            x2 = logits.double().requires_grad_(True)
            lq = F.log_softmax(x2, dim=-1)
            w = torch.cat([torch.tensor([0.4]), (0.1 / (C - 1)) * torch.ones(C - 1)]).double()
            total = F.ctc_loss(lq, targets, torch.full((N,), T, dtype=torch.int64), lengths, reduction="mean") - (lq * w).mean()
            total.backward()
            out[name + "/total64"] = np.float64(total.item())
            out[name + "/total_grad_logits64"] = x2.grad.numpy().copy()
        print(name, "nll64", true.numpy(), "ref32", out[name + "/ref32"], "ref16", out[name + "/ref16"])
    inf = np.isinf(out["t48_inf/nll64"])
    assert inf.sum() == 3 and np.isfinite(out["t48_c5/nll64"]).all() and np.isfinite(out["t40_c2/nll64"]).all()
    path = os.path.join(HERE, "ctc_loss.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

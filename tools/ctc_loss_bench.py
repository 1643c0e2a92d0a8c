#!/usr/bin/env python3
"""Time the CTC loss kernel (bonito_amd/csrc/ctc_loss.hip) against the only thing a user could have called before it:
torch.nn.functional.ctc_loss on the same device, forward and forward + backward (int64 targets, so that torch's native kernels are
the ones timed).

    python tools/ctc_loss_bench.py [--N 256 --T 1334 --min-len 225 --max-len 675 --iters 20 --warmup 3 --repeats 5 --out FILE]

The bonito.ctc training shape: fp32 log_softmax of seeded random logits, N = 256 chunks of T = 1334 steps (chunk 4000 at stride 3),
C = 5, target lengths uniform in [225, 675]. HIP events on the current stream around `iters` back-to-back launches after `warmup`
launches; the figure is the MEDIAN over `repeats` such measurements. bh_ctc_loss and bh_ctc_loss_grad are called through the C ABI with
buffers allocated once (nll, the label-smoothing numerator and - in the gradient entry - the gradient from one launch);
decode.ctc_nll_grad and Model.loss(...).backward() are timed as well, with their allocations. No threshold is set. Prints one JSON
object and writes it to --out (default profiles/ctc_loss_bench.json)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bonito_amd import _lib, decode  # noqa: E402


def timed(fn, iters, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--T", type=int, default=1334)
    ap.add_argument("--C", type=int, default=5)
    ap.add_argument("--min-len", type=int, default=225)
    ap.add_argument("--max-len", type=int, default=675)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctc_loss_bench.json"))
    args = ap.parse_args()
    N, T, Cn = args.N, args.T, args.C
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(25)
    lp = torch.log_softmax(torch.empty((T, N, Cn), dtype=torch.float32, device=dev).normal_(0.0, 2.0, generator=g), dim=-1)
    rng = np.random.default_rng(25)
    lengths = rng.integers(args.min_len, args.max_len + 1, size=N).astype(np.int32)
    Lmax = int(lengths.max())
    targets = rng.integers(1, Cn, size=(N, Lmax)).astype(np.int8)
    targets[np.arange(Lmax)[None, :] >= lengths[:, None]] = 0
    tg, ln = torch.from_numpy(targets).to(dev), torch.from_numpy(lengths).to(dev)
    w = torch.cat([torch.tensor([0.4]), (0.1 / (Cn - 1)) * torch.ones(Cn - 1)]).to(dev)

    lib = _lib.lib()
    st = _lib.stream_ptr(dev)
    ws_f = torch.empty(lib.bh_ctc_loss_workspace(N, T, Cn, Lmax), dtype=torch.uint8, device=dev)
    ws_g = torch.empty(lib.bh_ctc_loss_grad_workspace(N, T, Cn, Lmax), dtype=torch.uint8, device=dev)
    nll = torch.empty(N, dtype=torch.float32, device=dev)
    smooth = torch.empty(N, dtype=torch.float32, device=dev)
    grad = torch.empty_like(lp)
    head = (_lib.ptr(lp), 1, N, T, Cn, lp.stride(0), lp.stride(1), _lib.ptr(tg), Lmax, 1, _lib.ptr(ln), _lib.ptr(w))

    def forward():
        _lib.check(lib.bh_ctc_loss(*head, _lib.ptr(ws_f), _lib.ptr(nll), _lib.ptr(smooth), st), "bh_ctc_loss")

    def forward_grad():
        _lib.check(lib.bh_ctc_loss_grad(*head, None, None, _lib.ptr(ws_g), _lib.ptr(nll), _lib.ptr(smooth), _lib.ptr(grad),
                                        grad.stride(0), grad.stride(1), 1, 0, st), "bh_ctc_loss_grad")

    rep = (args.iters, args.warmup, args.repeats)
    ms_fwd, all_fwd = timed(forward, *rep)
    ms_grad, all_grad = timed(forward_grad, *rep)
    instance = int(lib.bh_ctc_loss_last_kernel())
    kernel_nll, kernel_grad = nll.clone(), grad.clone()
    ms_wrapper, _ = timed(lambda: decode.ctc_nll_grad(lp, tg, ln, w, layout="TNC"), *rep)

    from bonito_amd.ctc.model import Model
    xg = lp.clone().requires_grad_(True)

    def model_loss_backward():
        xg.grad = None
        Model.ctc_label_smoothing_loss(None, xg, tg, ln)["total_loss"].backward()

    ms_model, _ = timed(model_loss_backward, *rep)

    # torch on the same device: the native kernels (int64 targets), forward and forward + backward
    tg64, ln64 = tg.long(), ln.long()
    il = torch.full((N,), T, dtype=torch.int64, device=dev)
    xt = lp.clone().requires_grad_(True)

    def torch_forward():
        with torch.no_grad():
            return F.ctc_loss(lp, tg64, il, ln64, reduction="none")

    def torch_forward_backward():
        xt.grad = None
        F.ctc_loss(xt, tg64, il, ln64, reduction="sum").backward()

    ms_tf, all_tf = timed(torch_forward, *rep)
    ms_tb, all_tb = timed(torch_forward_backward, *rep)
    torch_nll = torch_forward()
    torch_forward_backward()
    torch_occ = lp.exp() - xt.grad                                          # torch returns exp(lp) - occ
    fin = torch.isfinite(torch_nll)

    res = {
        "shape": {"N": N, "T": T, "C": Cn, "min_len": args.min_len, "max_len": args.max_len, "Lmax": Lmax,
                  "mean_target_length": float(lengths.mean()), "log_probs": "fp32 [T, N, C]"},
        "instance": instance,
        "ms_bh_ctc_loss": ms_fwd, "ms_bh_ctc_loss_grad": ms_grad,
        "ms_decode_ctc_nll_grad_with_allocations": ms_wrapper, "ms_model_loss_forward_backward": ms_model,
        "ms_torch_ctc_loss_forward": ms_tf, "ms_torch_ctc_loss_forward_backward": ms_tb,
        "speedup_forward_vs_torch": ms_tf / ms_fwd, "speedup_forward_backward_vs_torch": ms_tb / ms_grad,
        "repeats_ms": {"bh_ctc_loss": all_fwd, "bh_ctc_loss_grad": all_grad, "torch_forward": all_tf, "torch_forward_backward": all_tb},
        "max_abs_difference_nll_kernel_vs_torch_fp32": float((kernel_nll - torch_nll)[fin].abs().max()),
        "max_abs_difference_occupancy_kernel_vs_torch_fp32": float((-kernel_grad - torch_occ)[:, fin].abs().max()),
        "finite_chunks": int(fin.sum()),
        "workspace_bytes": {"forward": int(ws_f.numel()), "gradient_alpha": int(ws_g.numel())},
        "bytes": {"log_probs": lp.numel() * 4, "gradient": grad.numel() * 4, "alpha_written_and_read_back": 2 * (int(ws_g.numel()) - 512)},
        "iters": args.iters, "warmup": args.warmup, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
    }
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time the CTC-CRF sequence scans (bonito_amd/csrc/seqdist.hip) against the only alternative a user had before them: the
reference's two gathers (CTC_CRF.prepare_ctc_scores, [T, N, L] fp32 stay / move tensors) followed by a torch scan over T on the
same device.

    python tools/seqdist_bench.py [--N 512 --T 1667 --state-len 5 --mean-len 400 --iters 50 --warmup 5 --out FILE]
    python tools/seqdist_bench.py --grad [--out profiles/seqdist_grad_bench.json]

--grad times the loss WITH its gradient instead: bh_crf_seq_logz_grad (logz and the posterior edge occupancy from one launch), the dense
posteriors, and CTC_CRF.ctc_loss(...).backward() end to end, against the same torch baseline with its autograd backward (reachable
targets only: that restatement's backward is NaN where a position cannot be reached). No threshold is set.

HIP events on the current stream around `iters` back-to-back launches after `warmup` launches; seeded random fp16 scores in the
engine's [N, T, 4S] layout; target lengths uniform in [mean/2, 3 mean/2]. Prints one JSON object (and writes it to --out).
Bytes: what the kernel must touch per call = two gathered fp16 values per (step, position) (whole 64-byte sectors in practice: up
to the full score tensor), plus one traceback bit per cell written and read back for the Max scan; the baseline writes and reads
2 x T x N x L x 4 bytes of gathered edges on top of that.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bonito_amd import _lib, decode  # noqa: E402
from bonito_amd.crf.model import CTC_CRF  # noqa: E402


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def torch_baseline(sd, x5, targets, n):
    """prepare_ctc_scores + the Log scan, all torch ops on the device (what koi.ctc.logZ_cu would have to be replaced by)."""
    stay, move = sd.prepare_ctc_scores(x5, targets)
    T, N, L = stay.shape
    alpha = stay.new_full((N, L), -float("inf"))
    alpha[:, 0] = 0.0
    pad = stay.new_full((N, 1), -float("inf"))
    for t in range(T):
        alpha = torch.logaddexp(alpha + stay[t], torch.cat([pad, alpha[:, :-1] + move[t]], dim=1))
    return alpha.gather(1, (n - 1)[:, None])[:, 0]


def grad_bench(args, x4, tg, ln, lengths, Lmax):
    N, T, sl = args.N, args.T, args.state_len
    S = 4 ** sl
    dev = x4.device
    sd = CTC_CRF(sl, ["N", "A", "C", "G", "T"])
    grad = torch.empty_like(x4)
    ms_chain = timed(lambda: decode.seq_logz_grad(x4, tg, ln, sl, 2.0, out=grad), args.iters, args.warmup)
    kernel_logz, _ = decode.seq_logz_grad(x4, tg, ln, sl, 2.0, out=grad)
    kernel_grad = grad.float()
    ms_dense = timed(lambda: decode.logz_grad(x4, sl, 2.0, out=grad), args.iters, args.warmup)
    xg = x4.clone().requires_grad_(True)

    def loss_and_backward():
        xg.grad = None
        sd.ctc_loss(xg, tg, ln, blank_score=2.0).backward()

    ms_loss = timed(loss_and_backward, args.iters, args.warmup)
    x5 = torch.nn.functional.pad(x4.view(N, T, S, 4), (1, 0), value=2.0).view(N, T, 5 * S).permute(1, 0, 2).contiguous()
    x5.requires_grad_(True)
    tg64, n64 = tg.long(), ln.long() + 1 - sl

    def baseline():
        x5.grad = None
        val = torch_baseline(sd, x5, tg64, n64)
        val.sum().backward()
        return val

    base_val = baseline().detach()
    base_grad = x5.grad.permute(1, 0, 2).reshape(N, T, S, 5)[..., 1:].reshape(N, T, 4 * S)
    agree = float((base_grad - kernel_grad).abs().max())
    ms_base = timed(baseline, args.baseline_iters, 1)
    return {
        "shape": {"N": N, "T": T, "state_len": sl, "mean_target_length": float(lengths.mean()), "Lmax": Lmax},
        "ms_seq_logz_grad": ms_chain, "ms_logz_dense_grad": ms_dense, "ms_ctc_loss_forward_backward": ms_loss,
        "ms_torch_gather_scan_autograd": ms_base, "speedup_seq_logz_grad_vs_torch_autograd": ms_base / ms_chain,
        "max_abs_difference_gradient_kernel_fp16_vs_torch_fp32": agree,
        "max_abs_difference_logz_kernel_vs_torch_fp32": float((base_val - kernel_logz).abs().max()),
        "workspace_bytes": {"chain_alpha": int(_lib.lib().bh_crf_seq_grad_workspace(N, T, Lmax, sl)),
                            "dense_alpha": int(_lib.lib().bh_crf_logz_dense_grad_workspace(N, T, sl))},
        "iters": args.iters, "warmup": args.warmup, "baseline_iters": args.baseline_iters, "device": torch.cuda.get_device_name(0),
    }


def emit(res, out):
    text = json.dumps(res, indent=1)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=512)
    ap.add_argument("--T", type=int, default=1667)
    ap.add_argument("--state-len", type=int, default=5)
    ap.add_argument("--mean-len", type=int, default=400)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--baseline-iters", type=int, default=3)
    ap.add_argument("--grad", action="store_true", help="time the loss with its gradient against torch autograd")
    ap.add_argument("--out")
    args = ap.parse_args()
    N, T, sl = args.N, args.T, args.state_len
    S = 4 ** sl
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(25)
    x4 = torch.empty((N, T, 4 * S), dtype=torch.float16, device=dev).normal_(0.0, 2.0, generator=g).clamp_(-5, 5)
    rng = np.random.default_rng(25)
    lengths = rng.integers(args.mean_len // 2, args.mean_len * 3 // 2 + 1, size=N).astype(np.int32)
    Lmax = int(lengths.max())
    targets = rng.integers(1, 5, size=(N, Lmax)).astype(np.int8)
    targets[np.arange(Lmax)[None, :] >= lengths[:, None]] = 0
    tg, ln = torch.from_numpy(targets).to(dev), torch.from_numpy(lengths).to(dev)

    if args.grad:
        emit(grad_bench(args, x4, tg, ln, lengths, Lmax), args.out)
        return

    lib = _lib.lib()
    ws = torch.empty(lib.bh_crf_seq_workspace(N, T, Lmax, sl), dtype=torch.uint8, device=dev)
    out = torch.empty(N, dtype=torch.float32, device=dev)
    align = torch.empty((N, T), dtype=torch.int32, device=dev)
    st = _lib.stream_ptr(dev)
    common = (_lib.ptr(x4), N, T, sl, 0, 2.0, T * 4 * S, 4 * S, _lib.ptr(tg), Lmax, 1, _lib.ptr(ln), _lib.ptr(ws))

    def log_scan():
        _lib.check(lib.bh_crf_seq_logz(*common, _lib.ptr(out), st), "bh_crf_seq_logz")

    def max_scan():
        _lib.check(lib.bh_crf_seq_viterbi(*common, _lib.ptr(align), _lib.ptr(out), st), "bh_crf_seq_viterbi")

    def free_scan():
        _lib.check(lib.bh_crf_seq_logz_free(_lib.ptr(x4), N, T, sl, 2.0, T * 4 * S, 4 * S, _lib.ptr(tg), Lmax, 1, _lib.ptr(ln),
                                            _lib.ptr(ws), _lib.ptr(out), st), "bh_crf_seq_logz_free")

    ms_log = timed(log_scan, args.iters, args.warmup)
    kernel_val = out.clone()
    ms_max = timed(max_scan, args.iters, args.warmup)
    ms_free = timed(free_scan, args.iters, args.warmup)

    # the baseline works on the reference layout [T, N, 5S] in fp32 chunks of the gather; built once, outside the timed region
    sd = CTC_CRF(sl, ["N", "A", "C", "G", "T"])
    x5 = torch.nn.functional.pad(x4.view(N, T, S, 4), (1, 0), value=2.0).view(N, T, 5 * S).permute(1, 0, 2)
    tg64, n64 = tg.long(), ln.long() + 1 - sl
    base_val = torch_baseline(sd, x5, tg64, n64)
    ms_base = timed(lambda: torch_baseline(sd, x5, tg64, n64), args.baseline_iters, 1)
    agree = float((base_val - kernel_val).abs().max())

    pos = int((lengths + 1 - sl).sum())
    res = {
        "shape": {"N": N, "T": T, "state_len": sl, "mean_target_length": float(lengths.mean()), "Lmax": Lmax},
        "ms_log_scan": ms_log, "ms_max_scan_with_traceback": ms_max, "ms_free_start_log_scan": ms_free,
        "ms_torch_gather_plus_scan": ms_base, "speedup_log_scan_vs_torch": ms_base / ms_log,
        "max_abs_difference_kernel_vs_torch_fp32": agree,
        "bytes": {"score_tensor": x4.numel() * 2, "gathered_values_min": 2 * 2 * T * pos,
                  "traceback_bits": int(ws.numel()) - 512,
                  "baseline_gathered_edges": 2 * T * N * (Lmax + 1 - sl) * 4},
        "iters": args.iters, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
    }
    emit(res, args.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Time bonito_amd.optim.AdamW.step(max_norm=2.0) (csrc/optim.hip: partial sums, finalise, update) on the parameter sets of the old-style
CRF model at 96 / 384 / 1024 features, beside torch's own path on the same device and tensors, and give the optimizer's share of a
whole training step.

    python tools/optim_bench.py [--features 96,384,1024 --N 64 --L 3000 --window 0.5 --repeats 5 --out FILE]

Per parameter set:
  ms_step          one AdamW.step(max_norm=2.0): sumsq launches + finalise + update launches, no synchronisation inside
  bytes            32 per element: 4 read in the norm pass, 16 read (p, g, m, v) and 12 written (p, m, v) in the update
  gbytes_per_s     bytes / ms_step;  share_of_hbm_peak = that over the 8.0 TB/s of the HBM3E specification. Back-to-back steps run on the
                   same tensors, so a set smaller than the 256 MiB last-level cache is served from it, not from HBM: for those sets
                   the figure is a rate, not a share of HBM bandwidth, and `fits_last_level_cache` says so.
  ms_torch         GradScaler.unscale_ + clip_grad_norm_(2.0) + GradScaler.step(torch.optim.AdamW(fused=True)) + GradScaler.update on
                   clones of the same tensors. GradScaler.step reads its overflow flag on the host, so this path synchronises once per
                   step; unscale_ divides the gradients in place, so they shrink from call to call (the work does not).
  ms_train_step    forward_train -> loss -> backward at N chunks of L samples (T = L / 5), as tools/train_step_bench.py times it
  optimizer_share  ms_step / (ms_train_step + ms_step)

Timing follows tools/train_step_bench.py: warm-up calls, a window of back-to-back calls of at least --window seconds between two HIP events,
the MEDIAN over --repeats windows. No threshold is set. Prints one JSON line and writes it to --out (default profiles/optim_bench.json)."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bonito_amd import optim  # noqa: E402
from bonito_amd.crf.model import Model  # noqa: E402
from train_step_bench import NOT_MEASURED, STATE_LEN  # noqa: E402

HBM_PEAK_BYTES_PER_S = 8.0e12
LAST_LEVEL_CACHE_BYTES = 256 << 20


def timed(fn, window, repeats):
    """train_step_bench.timed with room for a call of a few microseconds: up to 20000 calls per window."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(10):
        fn()
    b.record()
    b.synchronize()
    iters = max(1, min(20000, int(math.ceil(window * 1e3 / max(a.elapsed_time(b) / 10, 1e-3)))))
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out)


def attempt(fn, window, repeats):
    try:
        return timed(fn, window, repeats)
    except Exception as exc:
        if "HIP error" in str(exc):
            raise
        return "%s (%s: %s)" % (NOT_MEASURED, type(exc).__name__, str(exc)[:200])


def model_of(features, dev):
    torch.manual_seed(5)
    return Model({"labels": {"labels": ["N", "A", "C", "G", "T"]}, "global_norm": {"state_len": STATE_LEN.get(features, 3)},
                  "input": {"features": 1},
                  "encoder": dict(features=features, stride=5, winlen=19, scale=5.0, blank_score=2.0, num_layers=5, first_conv_size=4)}).to(dev)


def bench(features, N, L, window, repeats, dev):
    model = model_of(features, dev)
    params = [p for p in model.parameters() if p.requires_grad]
    g = torch.Generator(device=dev).manual_seed(41)
    for p in params:
        p.grad = torch.empty_like(p).normal_(0.0, 65536.0 * 1e-3, generator=g)
    elements = sum(p.numel() for p in params)
    res = {"features": features, "tensors": len(params), "elements": elements, "bytes": 32 * elements,
           "fits_last_level_cache": 16 * elements <= LAST_LEVEL_CACHE_BYTES}

    ours = optim.AdamW(params, lr=2e-3)
    res["ms_step"] = attempt(lambda: ours.step(max_norm=2.0), window, repeats)
    grad_norm, scale, skipped = ours.last()
    res["last"] = {"grad_norm": grad_norm, "scale": scale, "skipped": skipped}
    if isinstance(res["ms_step"], float):
        res["gbytes_per_s"] = res["bytes"] / res["ms_step"] / 1e6
        res["share_of_hbm_peak"] = res["bytes"] / (res["ms_step"] * 1e-3) / HBM_PEAK_BYTES_PER_S

    theirs_params = [torch.nn.Parameter(p.detach().clone()) for p in params]
    for q, p in zip(theirs_params, params):
        q.grad = p.grad.clone()
    theirs = torch.optim.AdamW(theirs_params, lr=2e-3, fused=True)
    scaler = torch.amp.GradScaler("cuda")
    scaler.scale(torch.zeros(1, device=dev))                  # creates the scale tensor

    def torch_step():
        scaler.unscale_(theirs)
        torch.nn.utils.clip_grad_norm_(theirs_params, 2.0)
        scaler.step(theirs)
        scaler.update()

    res["ms_torch"] = attempt(torch_step, window, repeats)
    del theirs, theirs_params, scaler

    x = torch.empty((N, 1, L), device=dev).normal_(generator=g).half()
    bases = L // 12
    targets = torch.randint(1, 5, (N, bases), generator=torch.Generator().manual_seed(6))
    lengths = torch.full((N,), bases, dtype=torch.int64)

    def train_step():
        for p in params:
            p.grad = None
        model.loss(model.forward_train(x), targets, lengths).backward()

    res["ms_train_step"] = attempt(train_step, window, repeats)
    if isinstance(res["ms_step"], float) and isinstance(res["ms_train_step"], float):
        res["optimizer_share"] = res["ms_step"] / (res["ms_train_step"] + res["ms_step"])
    else:
        res["optimizer_share"] = NOT_MEASURED
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", default="96,384,1024")
    ap.add_argument("--N", type=int, default=64)
    ap.add_argument("--L", type=int, default=3000)
    ap.add_argument("--window", type=float, default=0.5, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_bench: no HIP device; nothing is measured without one")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "repeats": args.repeats, "N": args.N, "L": args.L, "sets": []}
    for features in (int(v) for v in args.features.split(",")):
        res["sets"].append(bench(features, args.N, args.L, args.window, args.repeats, dev))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

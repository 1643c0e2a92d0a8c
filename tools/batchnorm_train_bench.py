#!/usr/bin/env python3
"""Time batch-statistics BatchNorm for training (bh_batchnorm_train_forward / _backward, csrc/batchnorm_train.hip) on the five
convolution outputs of the v5 `sup` stack - 64, 64, 128, 128, 512 channels at 12000, 12000, 4000, 2000, 1000 positions of a 12000-sample
chunk - for N = 16 and 64 chunks, each beside torch's fp16 F.batch_norm(training=True) + silu with autograd on the same device (in torch's
own [N][C][L] layout): the only thing a user could have called before. Then a whole forward_train -> loss -> backward of the v5-shaped
model with norm = "batchnorm" on every convolution (forward_train(norm="batch")) and with the norms taken off.

    python tools/batchnorm_train_bench.py [--N 16,64 --seconds 0.3 --repeats 5 --no-torch --no-model --out FILE]

Inputs are seeded. The layer is called through the C ABI with every buffer allocated once (at tens of microseconds a call the autograd
wrapper's host time would be the figure); torch's legs and the model run through autograd, as a user calls them. Each leg is warmed up
with one call, which also sizes the timed window: `iters` back-to-back calls that take at least --seconds between two HIP events on the
current stream; the figure is the MEDIAN over --repeats windows, and the legs alternate so that a drift of the shared host hits all.

Counted from the shape alone (swish, no clamp): the forward reads z three times (sum, centred sum, normalise) and writes y, 4 M C halves;
the backward reads z and dy twice each and writes dz, 5 M C halves (a clamp adds two reads of y). `*_gbytes_per_s` is that count over the
time, `*_share_of_copy` the same against the 6.29 TB/s a float4 copy reaches on this device. Tensors below the
256 MiB Infinity Cache are re-read from it, so a share above 1 is possible and says so. No time is fixed in advance. The result is rewritten
after every case. Prints one JSON line and writes it to --out (default profiles/batchnorm_train_bench.json)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bonito_amd import _lib  # noqa: E402
from transformer_train_bench import DEPTH, model_config, timed  # noqa: E402

CASES = ((64, 12000), (64, 12000), (128, 4000), (128, 2000), (512, 1000))          # (channels, positions) behind each v5 convolution
EPS, MOMENTUM, COPY_TBYTES_PER_S = 1e-5, 0.1, 6.29
INF = float("inf")


def bench_case(N, L, C, seconds, repeats, with_torch, dev):
    M = N * L
    g = torch.Generator(device=dev).manual_seed(47)
    rand = lambda *s: torch.empty(s, dtype=torch.float32, device=dev).normal_(generator=g)      # noqa: E731
    z, dy = (rand(N, L, C) * 1.5 + 0.25).half(), rand(N, L, C).half()
    gamma, beta = 1.0 + 0.1 * rand(C), 0.1 * rand(C)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    y, dz = torch.empty_like(z), torch.empty_like(z)
    mean, rstd, dgamma, dbeta = (torch.empty(C, dtype=torch.float32, device=dev) for _ in range(4))
    lib, st = _lib.lib(), _lib.stream_ptr(dev)
    nbytes = lib.bh_batchnorm_train_workspace(N, L, C)
    if nbytes == 0:
        raise SystemExit("batchnorm_train_bench: shape N=%d L=%d C=%d is not served" % (N, L, C))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    act = _lib.BH_ACT["swish"]

    def forward():
        _lib.check(lib.bh_batchnorm_train_forward(_lib.ptr(z), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(rm), _lib.ptr(rv), N, L, C, C, EPS, MOMENTUM,
                                                  act, -INF, INF, L * C, C, _lib.ptr(y), _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(ws), nbytes, st),
                   "bh_batchnorm_train_forward")

    def both():
        forward()
        _lib.check(lib.bh_batchnorm_train_backward(_lib.ptr(z), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(y),
                                                   _lib.ptr(dy), N, L, C, C, act, -INF, INF, L * C, C, _lib.ptr(dz), _lib.ptr(dgamma), _lib.ptr(dbeta),
                                                   _lib.ptr(ws), nbytes, st), "bh_batchnorm_train_backward")

    legs = {"forward": forward, "forward_backward": both}
    if with_torch:
        tz = z.permute(0, 2, 1).contiguous().requires_grad_()
        tdy = dy.permute(0, 2, 1).contiguous()
        tg, tb = gamma.half().requires_grad_(), beta.half().requires_grad_()
        trm, trv = rm.half(), rv.half()
        layer = lambda: torch.nn.functional.silu(torch.nn.functional.batch_norm(tz, trm, trv, tg, tb, True, MOMENTUM, EPS))      # noqa: E731

        def torch_forward():
            with torch.no_grad():
                return layer()

        def torch_both():
            tz.grad = tg.grad = tb.grad = None
            layer().backward(tdy)

        legs.update(torch_forward=torch_forward, torch_forward_backward=torch_both)
    ms, reps, iters = timed(legs, seconds, repeats)
    res = {"N": N, "L": L, "C": C, "mbytes_z": M * C * 2 / 1e6, "repeats_ms": reps, "iters": iters}
    res.update({"ms_" + k: v for k, v in ms.items()})
    res["ms_backward"] = ms["forward_backward"] - ms["forward"]
    for name, halves in (("forward", 4), ("backward", 5)):
        rate = halves * M * C * 2 / res["ms_" + name] / 1e6
        res[name + "_gbytes_per_s"], res[name + "_share_of_copy"] = rate, rate / (COPY_TBYTES_PER_S * 1e3)
    if with_torch:
        res["ms_torch_backward"] = ms["torch_forward_backward"] - ms["torch_forward"]
        res["speedup_forward_vs_torch"] = ms["torch_forward"] / ms["forward"]
        res["speedup_forward_backward_vs_torch"] = ms["torch_forward_backward"] / ms["forward_backward"]
        both()
        torch_both()
        torch.cuda.synchronize()
        rel = lambda a, b: float((a.float() - b.float()).abs().max() / b.float().abs().max())      # noqa: E731
        res["difference_vs_torch"] = {"y": rel(y, torch_forward().permute(0, 2, 1)), "dz": rel(dz, tz.grad.permute(0, 2, 1)),
                                      "dgamma": rel(dgamma, tg.grad), "dbeta": rel(dbeta, tb.grad)}
    return res


def bench_model(N, T, seconds, repeats, dev, norm):
    from bonito_amd.transformer import Model
    config = model_config()
    if norm:
        for layer in config["model"]["encoder"]["conv"]["sublayers"][:5]:
            layer["norm"] = "batchnorm"
    torch.manual_seed(7)
    model = Model(config).to(dev).train()
    kw = {"norm": "batch"} if norm else {}
    L = 12 * T
    g = torch.Generator().manual_seed(45)
    x = torch.randn(N, 1, L, generator=g).half().to(dev)
    lengths = torch.randint(L // 24, L // 12, (N,), generator=g)
    targets = torch.randint(1, 5, (N, int(lengths.max())), generator=g)
    params = list(model.parameters())

    def forward():
        with torch.no_grad():
            model.forward_train(x, **kw)

    def step():
        for p in params:
            p.grad = None
        model.loss(model.forward_train(x, **kw), targets, lengths).backward()

    ms, reps, iters = timed({"forward_train": forward, "step": step}, seconds, repeats)
    return {"N": N, "samples": L, "T": T, "depth": DEPTH, "norm": "batchnorm" if norm else None, "ms_forward_train": ms["forward_train"],
            "ms_step": ms["step"], "repeats_ms": reps, "iters": iters,
            "finite": all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params if p.requires_grad)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", default="16,64")
    ap.add_argument("--seconds", type=float, default=0.3, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batchnorm_train_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("batchnorm_train_bench: no HIP device; nothing is measured without one")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "seconds": args.seconds, "repeats": args.repeats, "copy_tbytes_per_s": COPY_TBYTES_PER_S,
           "cases": []}

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")

    for N in (int(v) for v in args.N.split(",")):
        for C, L in CASES:
            res["cases"].append(bench_case(N, L, C, args.seconds, args.repeats, not args.no_torch, dev))
            write()
            torch.cuda.empty_cache()
    if not args.no_model:
        res["model"] = [bench_model(16, 1000, args.seconds, args.repeats, dev, norm) for norm in (False, True)]
        write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

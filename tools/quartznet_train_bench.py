#!/usr/bin/env python3
"""Time what training a QuartzNet CTC model adds (csrc/quartznet_train.hip).

1. The depthwise backward (bh_dwconv1d_train_backward: dx and dw) at the six separable shapes of dna_r9.4.1@v2 - (C, K) = (424, 115),
   (464, 5), (456, 123), (440, 9), (280, 31), (384, 67) at L = 1200 positions - for N = 32 and 128 chunks, each beside torch's fp16
   F.conv1d(groups=C) with autograd on the same device (torch's own [N][C][L] layout): the only thing a user could have called before.
2. A whole forward_train(norm="batch") -> loss -> backward of the dna_r9.4.1@v2 configuration (tests/golden/configs) on chunks of 3600
   samples, beside a restatement of the same network in torch fp16 modules (Conv1d, BatchNorm1d, SiLU, Dropout, log_softmax) with
   torch.nn.functional.ctc_loss, with autograd.

    python tools/quartznet_train_bench.py [--N 32,128 (--N "" skips the layer cases) --model-N 32 --seconds 0.3 --repeats 5 --no-torch --no-model --out FILE]

Inputs are seeded. The layer is called through the C ABI with every buffer allocated once; torch's legs and the model run through
autograd, as a user calls them. Each leg is warmed up with one call, which also sizes the timed window: `iters` back-to-back calls that
take at least --seconds between two HIP events on the current stream; the figure is the MEDIAN over --repeats windows, and the legs
alternate so that a drift of the shared host hits all.

Counted from the shape alone: dx and dw are each N Lout C K fused multiply-adds - `share_of_fma_peak` is 2 N Lout C K FMAs over the time
against the 78.65e12 fp32 FMA/s (157.3 TFLOP/s) of the vector ALUs - and the layer reads x and dy and writes dx once, 3 N L C halves:
`share_of_copy` is that count over the time against the 6.29 TB/s a float4 copy reaches on this device. No time is
fixed in advance. The result is rewritten after every case. Prints one JSON line and writes it to --out (default
profiles/quartznet_train_bench.json)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bonito_amd import _lib  # noqa: E402
from transformer_train_bench import timed  # noqa: E402

CASES = ((424, 115), (464, 5), (456, 123), (440, 9), (280, 31), (384, 67))          # (channels, taps) of @v2's separable blocks
L = 1200
FMA_PER_S, COPY_TBYTES_PER_S = 78.65e12, 6.29


def bench_case(N, C, K, seconds, repeats, with_torch, dev):
    pad = K // 2
    g = torch.Generator(device=dev).manual_seed(47)
    rand = lambda *s: torch.empty(s, dtype=torch.float32, device=dev).normal_(generator=g)      # noqa: E731
    x, dy, w = rand(N, L, C).half(), rand(N, L, C).half(), rand(C, 1, K) / K ** 0.5
    dx, dw = torch.empty_like(x), torch.empty_like(w)
    lib, st = _lib.lib(), _lib.stream_ptr(dev)
    nbytes = lib.bh_dwconv1d_train_workspace(N, L, C, K, pad)
    if nbytes == 0:
        raise SystemExit("quartznet_train_bench: shape N=%d L=%d C=%d K=%d is not served" % (N, L, C, K))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)

    def call(dxp, dwp):
        _lib.check(lib.bh_dwconv1d_train_backward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(dy), N, L, C, K, pad, dxp, dwp, _lib.ptr(ws), nbytes, st),
                   "bh_dwconv1d_train_backward")

    legs = {"backward": lambda: call(_lib.ptr(dx), _lib.ptr(dw)), "dx": lambda: call(_lib.ptr(dx), None), "dw": lambda: call(None, _lib.ptr(dw))}
    if with_torch:
        tx = x.permute(0, 2, 1).contiguous().requires_grad_()
        tdy = dy.permute(0, 2, 1).contiguous()
        tw = w.half().requires_grad_()
        layer = lambda: torch.nn.functional.conv1d(tx, tw, padding=pad, groups=C)      # noqa: E731

        def torch_forward():
            with torch.no_grad():
                return layer()

        def torch_both():
            tx.grad = tw.grad = None
            layer().backward(tdy)

        legs.update(torch_forward=torch_forward, torch_forward_backward=torch_both)
    ms, reps, iters = timed(legs, seconds, repeats)
    fma = 2.0 * N * L * C * K
    res = {"N": N, "L": L, "C": C, "K": K, "workspace_mbytes": nbytes / 1e6, "repeats_ms": reps, "iters": iters}
    res.update({"ms_" + k: v for k, v in ms.items()})
    res["share_of_fma_peak"] = fma / (ms["backward"] * 1e-3) / FMA_PER_S
    res["dw_share_of_fma_peak"] = 0.5 * fma / (ms["dw"] * 1e-3) / FMA_PER_S
    res["dx_share_of_fma_peak"] = 0.5 * fma / (ms["dx"] * 1e-3) / FMA_PER_S
    res["share_of_copy"] = 3.0 * N * L * C * 2 / (ms["backward"] * 1e-3) / (COPY_TBYTES_PER_S * 1e12)
    if with_torch:
        res["ms_torch_backward"] = ms["torch_forward_backward"] - ms["torch_forward"]
        res["speedup_backward_vs_torch"] = res["ms_torch_backward"] / ms["backward"]
        call(_lib.ptr(dx), _lib.ptr(dw))
        torch_both()
        torch.cuda.synchronize()
        rel = lambda a, b: float((a.float() - b.float()).abs().max() / b.float().abs().max())      # noqa: E731
        res["difference_vs_torch"] = {"dx": rel(dx, tx.grad.permute(0, 2, 1)), "dw": rel(dw, tw.grad)}
    return res


class _TorchBlock(torch.nn.Module):
    """A QuartzNet block in torch modules, as bonito's ctc model builds it."""

    def __init__(self, cin, layer, act):
        super().__init__()
        nn = torch.nn
        cout, K, stride, mods = layer["filters"], layer["kernel"][0], layer["stride"][0], []
        c = cin
        for r in range(layer["repeat"]):
            if layer["separable"]:
                mods += [nn.Conv1d(c, c, K, stride=stride, padding=K // 2, groups=c, bias=False), nn.Conv1d(c, cout, 1, bias=False)]
            else:
                mods += [nn.Conv1d(c, cout, K, stride=stride, padding=K // 2, bias=False)]
            mods += [nn.BatchNorm1d(cout, eps=1e-3, momentum=0.1)]
            if r < layer["repeat"] - 1:
                mods += [act(), nn.Dropout(layer["dropout"])]
            c = cout
        self.conv = nn.Sequential(*mods)
        self.residual = nn.Sequential(nn.Conv1d(cin, cout, 1, bias=False), nn.BatchNorm1d(cout, eps=1e-3, momentum=0.1)) if layer["residual"] else None
        self.out = nn.Sequential(act(), nn.Dropout(layer["dropout"]))

    def forward(self, x):
        y = self.conv(x)
        return self.out(y if self.residual is None else y + self.residual(x))


def bench_model(N, samples, seconds, repeats, dev, with_torch):
    from bonito_amd.ctc import Model
    from bonito_amd.util import load_toml
    config = load_toml(os.path.join(ROOT, "tests", "golden", "configs", "dna_r9.4.1@v2.toml"))
    torch.manual_seed(7)
    model = Model(config).to(dev).train()
    g = torch.Generator().manual_seed(45)
    x = torch.randn(N, 1, samples, generator=g).half().to(dev)
    T = samples // config["block"][0]["stride"][0]
    lengths = torch.randint(T // 8, T // 4, (N,), generator=g)
    targets = torch.randint(1, 5, (N, int(lengths.max())), generator=g)
    params = list(model.parameters())

    def forward():
        with torch.no_grad():
            model.forward_train(x, norm="batch")

    def step():
        for p in params:
            p.grad = None
        model.loss(model.forward_train(x, norm="batch"), targets, lengths)["total_loss"].backward()

    legs = {"forward_train": forward, "step": step}
    if with_torch:
        blocks, c = [], 1
        for layer in config["block"]:
            blocks.append(_TorchBlock(c, layer, torch.nn.SiLU))
            c = layer["filters"]
        net = torch.nn.Sequential(*blocks, torch.nn.Conv1d(c, len(config["labels"]["labels"]), 1)).to(dev).half().train()
        tparams = list(net.parameters())
        tt, tl = targets.to(dev), lengths.to(dev)
        in_lengths = torch.full((N,), T, dtype=torch.int64, device=dev)

        def torch_step():
            for p in tparams:
                p.grad = None
            lp = torch.log_softmax(net(x), dim=1).permute(2, 0, 1)
            torch.nn.functional.ctc_loss(lp.float(), tt, in_lengths, tl, reduction="mean").backward()

        legs["torch_step"] = torch_step
    ms, reps, iters = timed(legs, seconds, repeats)
    res = {"N": N, "samples": samples, "T": T, "config": "dna_r9.4.1@v2", "repeats_ms": reps, "iters": iters,
           "finite": all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params if p.requires_grad)}
    res.update({"ms_" + k: v for k, v in ms.items()})
    if with_torch:
        res["speedup_step_vs_torch"] = ms["torch_step"] / ms["step"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", default="32,128")
    ap.add_argument("--model-N", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=0.3, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quartznet_train_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("quartznet_train_bench: no HIP device; nothing is measured without one")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "seconds": args.seconds, "repeats": args.repeats, "fma_per_s": FMA_PER_S,
           "copy_tbytes_per_s": COPY_TBYTES_PER_S, "cases": []}

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")

    for N in (int(v) for v in args.N.split(",") if v):
        for C, K in CASES:
            res["cases"].append(bench_case(N, C, K, args.seconds, args.repeats, not args.no_torch, dev))
            write()
            torch.cuda.empty_cache()
    if not args.no_model:
        res["model"] = bench_model(args.model_N, 3600, args.seconds, args.repeats, dev, not args.no_torch)
        write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

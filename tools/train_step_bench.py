#!/usr/bin/env python3
"""Time the training layers of an LSTM-family CRF model (bonito_amd/csrc/train_layers.hip through bonito_amd.train_ops) and the whole
training step SeqdistModel.forward_train -> loss -> backward, and give each new layer's share of the step.

    python tools/train_step_bench.py [--L 3000 --N 64,512 --features 96,384,1024 --window 0.3 --repeats 3 --no-torch --out FILE]

The model is the old-style rnn_encoder: conv 1 -> 4 -> 16 -> features (19 taps, stride 5, so T = L / 5 = 600), five LSTM layers, a
tanh x 5 head with 4^(state_len + 1) outputs (state_len 3 / 4 / 5 at 96 / 384 / 1024 features, as the fast / hac / sup models). The
layers are timed as forward_train calls them (the 4 channels between the first two convolutions zero-padded to 8; the third convolution
stores time-major): forward, and forward + backward through autograd with gradients for the input, the weight and the bias. Beside
each, torch's own fp16 conv1d + silu / linear + tanh autograd on the same device and the same shapes, where that runs; a cell that cannot
be taken reads "not measured" with the reason. torch's LSTM is never started by this tool (tools/lstm_train_bench.py does, and does
not from 2^31 bytes of gates on), so the whole step has no torch column.

Each timing is warmed up with one call, which also sizes the window: `iters` back-to-back calls taking at least --window seconds between
two HIP events; the figure is the MEDIAN over --repeats windows. No threshold is set. The result is rewritten after every shape. Prints
one JSON line and writes it to --out (default profiles/train_step_bench.json)."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bonito_amd import train_ops  # noqa: E402
from bonito_amd.crf.model import Model  # noqa: E402

STATE_LEN = {96: 3, 384: 4, 1024: 5}
NOT_MEASURED = "not measured"


def timed(fn, window, repeats):
    """-> median ms per call. One warm-up call; a second, timed on its own, sizes the window."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    iters = max(1, min(200, int(math.ceil(window * 1e3 / max(a.elapsed_time(b), 1e-3)))))
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


def bench_conv(name, N, Lin, Cin, Cout, K, stride, tm, window, repeats, with_torch, dev, g):
    pad = K // 2
    x = torch.empty((N, Lin, Cin) if Cin > 1 else (N, Lin), device=dev).normal_(generator=g).half()
    w = torch.empty((Cout, Cin, K), device=dev).normal_(0.0, 1.0 / math.sqrt(Cin * K), generator=g).requires_grad_()
    b = torch.empty(Cout, device=dev).normal_(0.0, 0.1, generator=g).requires_grad_()
    Lout = train_ops.conv_out_len(Lin, K, stride, pad)
    dy = torch.empty((Lout, N, Cout) if tm else (N, Lout, Cout), device=dev).normal_(generator=g).half()
    xg = x.clone().requires_grad_()

    def forward():
        with torch.no_grad():
            train_ops.conv1d(x, w, b, stride, pad, "swish", None, tm)

    def both():
        xg.grad = w.grad = b.grad = None
        train_ops.conv1d(xg, w, b, stride, pad, "swish", None, tm).backward(dy)

    res = {"layer": name, "shape": [N, Lin, Cin, Cout, K, stride], "ms_forward": attempt(forward, window, repeats),
           "ms_forward_backward": attempt(both, window, repeats), "ms_torch_forward": NOT_MEASURED, "ms_torch_forward_backward": NOT_MEASURED}
    if with_torch:
        xt = (x if Cin > 1 else x[:, :, None]).permute(0, 2, 1).contiguous().requires_grad_()
        wt, bt = w.detach().half().requires_grad_(), b.detach().half().requires_grad_()
        dyt = (dy.permute(1, 2, 0) if tm else dy.permute(0, 2, 1)).contiguous()

        def torch_forward():
            with torch.no_grad():
                torch.nn.functional.silu(torch.nn.functional.conv1d(xt, wt, bt, stride=stride, padding=pad))

        def torch_both():
            xt.grad = wt.grad = bt.grad = None
            torch.nn.functional.silu(torch.nn.functional.conv1d(xt, wt, bt, stride=stride, padding=pad)).backward(dyt)

        res["ms_torch_forward"] = attempt(torch_forward, window, repeats)
        res["ms_torch_forward_backward"] = attempt(torch_both, window, repeats)
    return res


def bench_head(T, N, K, C, window, repeats, with_torch, dev, g):
    x = torch.empty((T, N, K), device=dev).normal_(generator=g).half()
    w = torch.empty((C, K), device=dev).normal_(0.0, 1.0 / math.sqrt(K), generator=g).requires_grad_()
    b = torch.empty(C, device=dev).normal_(0.0, 0.1, generator=g).requires_grad_()
    dy = torch.empty((N, T, C), dtype=torch.float16, device=dev).normal_(generator=g)
    xg = x.clone().requires_grad_()

    def forward():
        with torch.no_grad():
            train_ops.linear(x, w, b, "tanh", 5.0, None, True)

    def both():
        xg.grad = w.grad = b.grad = None
        train_ops.linear(xg, w, b, "tanh", 5.0, None, True).backward(dy)

    res = {"layer": "head", "shape": [T, N, K, C], "ms_forward": attempt(forward, window, repeats),
           "ms_forward_backward": attempt(both, window, repeats), "ms_torch_forward": NOT_MEASURED, "ms_torch_forward_backward": NOT_MEASURED}
    if with_torch:
        wt, bt = w.detach().half().requires_grad_(), b.detach().half().requires_grad_()
        dyt = dy.permute(1, 0, 2).contiguous()

        def torch_forward():
            with torch.no_grad():
                torch.tanh(torch.nn.functional.linear(x, wt, bt)) * 5.0

        def torch_both():
            xg.grad = wt.grad = bt.grad = None
            (torch.tanh(torch.nn.functional.linear(xg, wt, bt)) * 5.0).backward(dyt)

        res["ms_torch_forward"] = attempt(torch_forward, window, repeats)
        res["ms_torch_forward_backward"] = attempt(torch_both, window, repeats)
    return res


def bench_step(N, L, features, window, repeats, dev, g):
    state_len = STATE_LEN.get(features, 3)
    torch.manual_seed(5)
    model = Model({"labels": {"labels": ["N", "A", "C", "G", "T"]}, "global_norm": {"state_len": state_len}, "input": {"features": 1},
                   "encoder": dict(features=features, stride=5, winlen=19, scale=5.0, blank_score=2.0, num_layers=5, first_conv_size=4)}).to(dev)
    x = torch.empty((N, 1, L), device=dev).normal_(generator=g).half()
    bases = L // 12                                        # about 0.42 bases per step of the stride-5 model
    targets = torch.randint(1, 5, (N, bases), generator=torch.Generator().manual_seed(6))
    lengths = torch.full((N,), bases, dtype=torch.int64)
    params = [p for p in model.parameters() if p.requires_grad]

    def forward():
        with torch.no_grad():
            model.forward_train(x)

    def step():
        for p in params:
            p.grad = None
        model.loss(model.forward_train(x), targets, lengths).backward()

    return {"ms_forward_train": attempt(forward, window, repeats), "ms_step": attempt(step, window, repeats), "state_len": state_len,
            "target_bases": bases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=3000)
    ap.add_argument("--N", default="64,512")
    ap.add_argument("--features", default="96,384,1024")
    ap.add_argument("--window", type=float, default=0.3, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_step_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_step_bench: no HIP device; nothing is measured without one")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "repeats": args.repeats, "L": args.L, "shapes": []}
    for features in (int(v) for v in args.features.split(",")):
        for N in (int(v) for v in args.N.split(",")):
            g = torch.Generator(device=dev).manual_seed(41)
            T = train_ops.conv_out_len(args.L, 19, 5, 9)
            a = (args.window, args.repeats, not args.no_torch, dev, g)
            layers = [bench_conv("conv0", N, args.L, 1, 8, 5, 1, False, *a), bench_conv("conv1", N, args.L, 8, 16, 5, 1, False, *a),
                      bench_conv("conv2", N, args.L, 16, features, 19, 5, True, *a),
                      bench_head(T, N, features, 4 ** (STATE_LEN.get(features, 3) + 1), *a)]
            shape = {"N": N, "T": T, "features": features, "layers": layers}
            shape.update(bench_step(N, args.L, features, args.window, args.repeats, dev, g))
            new = [r["ms_forward_backward"] for r in layers]
            if all(isinstance(v, float) for v in new) and isinstance(shape["ms_step"], float):
                shape["share_of_step"] = {r["layer"]: r["ms_forward_backward"] / shape["ms_step"] for r in layers}
                shape["share_of_step"]["conv_and_head"] = sum(new) / shape["ms_step"]
            else:
                shape["share_of_step"] = NOT_MEASURED
            res["shapes"].append(shape)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as fh:
                    fh.write(json.dumps(res) + "\n")
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

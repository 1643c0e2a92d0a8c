#!/usr/bin/env python3
"""Time one transformer encoder layer for training (bonito_amd.attn.encoder_layer: attention, the two DeepNorm residual RMSNorms and
the gated MLP; csrc/transformer_train.hip, attention_train.hip, train_layers.hip) at the v5 `sup` shape - d_model 512, 8 heads,
dim_feedforward 2048, window (127, 128) - its norm and its gated input layer alone, and a whole forward_train -> loss -> backward of the
18-layer model, each beside a torch fp16 restatement with autograd on the same device (scaled_dot_product_attention under the band mask
as in tools/attn_train_bench.py, RMSNorm and SwiGLU written in torch ops): the only thing a user could have called before.

    python tools/transformer_train_bench.py [--T 1000 --N 16,64 --seconds 0.5 --repeats 5 --no-torch --no-model --out FILE]

Inputs and weights are seeded. The layer and the model run through autograd, as a user calls them; the norm and the gated layer alone are
called through the C ABI with every buffer allocated once (at 0.1 ms a call the autograd wrapper's host time would be the figure), torch's
legs through its autograd throughout. Each leg is warmed up with one call, which also sizes the timed window: `iters` back-to-back calls that
take at least --seconds between two HIP events on the current stream; the figure is the MEDIAN over --repeats windows, and the legs
alternate (ours, torch, ours, ...) so that a drift of the shared host hits both.

Counted from the shape alone: the norm's backward moves 5 M D halves (a, x, dy in; da, dx out; the gain and dw are D floats), so
`norm_backward_gbytes_per_s` = 10 M D bytes over its time. The gated layer's backward recomputes u = x W1^T with the plain GEMM instead of
keeping M 2F halves per layer; that GEMM is timed alone and `gated_recompute_share` is its share of the backward - what a storing epilogue
would have to beat. No time is fixed in advance. The result is rewritten after every shape. Prints one JSON line and writes it to --out
(default profiles/transformer_train_bench.json)."""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bonito_amd import _lib, attn  # noqa: E402
from bonito_amd.transformer.model import TransformerEncoderLayer, deepnorm_params  # noqa: E402

D, H, F, WINDOW, DEPTH, EPS = 512, 8, 2048, (127, 128), 18, 1e-5
INF = float("inf")


def window_iters(fn, seconds):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return max(1, min(2000, int(math.ceil(seconds * 1e3 / max(a.elapsed_time(b), 1e-3)))))


def one_window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def timed(legs, seconds, repeats):
    """legs: {name: fn} -> {name: median ms}; the legs alternate inside every repeat."""
    iters = {k: window_iters(fn, seconds) for k, fn in legs.items()}
    out = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            out[k].append(one_window(fn, iters[k]))
    return {k: statistics.median(v) for k, v in out.items()}, out, iters


def rel(a, b):
    return float((a.float() - b.float()).abs().max() / b.float().abs().max())


def rms(z, w, eps=EPS):
    return z * torch.rsqrt(z.float().pow(2).mean(-1, keepdim=True) + eps).to(z.dtype) * w


def rotary(x, tab):
    """x [N, T, H, 64] fp16, tab [T, 32, 2] fp32 -> rotated, in torch ops (differentiable)."""
    cos, sin = tab[None, :, None, :, 0].to(x.dtype), tab[None, :, None, :, 1].to(x.dtype)
    x1, x2 = x[..., :32], x[..., 32:]
    return torch.cat([x1 * cos - x2 * sin, x1 * sin + x2 * cos], dim=-1)


def torch_layer(p, x, tab, mask, alpha):
    """The reference's TransformerEncoderLayer.forward in torch fp16 ops; p: fp16 leaves under the container's parameter names."""
    N, T, _ = x.shape
    lin = torch.nn.functional.linear
    qkv = lin(x, p["self_attn.Wqkv.weight"]).view(N, T, 3, H, 64)
    q, k, v = (t.permute(0, 2, 1, 3) for t in (rotary(qkv[:, :, 0], tab), rotary(qkv[:, :, 1], tab), qkv[:, :, 2]))
    o = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=mask).permute(0, 2, 1, 3).reshape(N, T, D)
    x1 = rms(lin(o, p["self_attn.out_proj.weight"], p["self_attn.out_proj.bias"]) + alpha * x, p["norm1.weight"])
    y, gate = lin(x1, p["ff.fc1.weight"]).chunk(2, dim=-1)
    return rms(lin(y * torch.nn.functional.silu(gate), p["ff.fc2.weight"]) + alpha * x1, p["norm2.weight"])


def grad_legs(name, fn, leaves, dy, legs):
    """forward under no_grad, and forward + backward with the leaves' gradients dropped first."""
    def forward():
        with torch.no_grad():
            return fn()

    def both():
        for t in leaves:
            t.grad = None
        fn().backward(dy)

    legs[name + "_forward"], legs[name + "_forward_backward"] = forward, both


def bench_shape(N, T, seconds, repeats, with_torch, dev):
    M = N * T
    g = torch.Generator(device=dev).manual_seed(43)
    rand = lambda *s: torch.empty(s, dtype=torch.float32, device=dev).normal_(generator=g)      # noqa: E731
    alpha, beta = deepnorm_params(DEPTH)
    torch.manual_seed(5)
    layer = TransformerEncoderLayer(D, H, F, alpha, beta, attn_window=WINDOW).to(dev)
    x, dy = rand(N, T, D).half().requires_grad_(), rand(N, T, D).half()
    a, dh = rand(N, T, D).half().requires_grad_(), rand(N, T, F).half()
    params = list(layer.parameters())
    legs = {}
    grad_legs("layer", lambda: attn.encoder_layer(layer, x), params + [x], dy, legs)
    # the norm and the gated layer alone: through the C ABI with every buffer allocated once, so that a kernel's time is not the host's
    lib, st = _lib.lib(), _lib.stream_ptr(dev)
    gain, w1 = layer.norm1.weight.detach(), layer.ff.fc1.weight.detach()
    ad, xd = a.detach(), x.detach()
    out, da, dx = (torch.empty_like(ad) for _ in range(3))
    h = torch.empty((N, T, F), dtype=torch.float16, device=dev)
    dgain, dw1 = torch.empty_like(gain), torch.empty_like(w1)
    nb, gb = lib.bh_rmsnorm_train_workspace(M, D), lib.bh_gated_linear_train_workspace(M, D, F)
    if nb == 0 or gb == 0:
        raise SystemExit("transformer_train_bench: shape M=%d D=%d F=%d is not served" % (M, D, F))
    nws, gws = torch.empty(nb, dtype=torch.uint8, device=dev), torch.empty(gb, dtype=torch.uint8, device=dev)

    def norm_forward():
        _lib.check(lib.bh_rmsnorm_residual(_lib.ptr(ad), _lib.ptr(xd), _lib.ptr(gain), _lib.ptr(out), M, D, alpha, EPS, st), "bh_rmsnorm_residual")

    def norm_both():
        norm_forward()
        _lib.check(lib.bh_rmsnorm_train_backward(_lib.ptr(ad), _lib.ptr(xd), _lib.ptr(gain), _lib.ptr(dy), M, D, alpha, EPS, _lib.ptr(da), _lib.ptr(dx),
                                                 _lib.ptr(dgain), _lib.ptr(nws), nb, st), "bh_rmsnorm_train_backward")

    def gated_forward():
        _lib.check(lib.bh_gated_linear_train_forward(_lib.ptr(xd), _lib.ptr(w1), M, D, F, _lib.ptr(h), _lib.ptr(gws), gb, st),
                   "bh_gated_linear_train_forward")

    def gated_both():
        gated_forward()
        _lib.check(lib.bh_gated_linear_train_backward(_lib.ptr(xd), _lib.ptr(w1), _lib.ptr(dh), M, D, F, _lib.ptr(dx), _lib.ptr(dw1), _lib.ptr(gws), gb,
                                                      st), "bh_gated_linear_train_backward")

    legs.update({"norm_forward": norm_forward, "norm_forward_backward": norm_both, "gated_forward": gated_forward,
                 "gated_forward_backward": gated_both})
    w16 = w1.half().contiguous()
    u = torch.empty((M, 2 * F), dtype=torch.float16, device=dev)

    def recompute():      # the GEMM the gated backward runs again: u = x W1^T, plain epilogue
        _lib.check(lib.bh_linear(_lib.ptr(x), _lib.ptr(w16), None, _lib.ptr(u), M, 2 * F, D, D, D, 2 * F, 0, 1.0, -INF, INF, 0, 0, 0, 0, 0, st),
                   "bh_linear")

    legs["gated_recompute_gemm"] = recompute
    if with_torch:
        tab_h = np.empty((T, 32, 2), np.float32)
        _lib.check(lib.bh_rotary_table(T, 64, tab_h.ctypes.data), "bh_rotary_table")
        tab = torch.from_numpy(tab_h).to(dev)
        i = torch.arange(T, device=dev)
        mask = (i[None, :] >= i[:, None] - WINDOW[0]) & (i[None, :] <= i[:, None] + WINDOW[1])
        p16 = {k: v.detach().half().requires_grad_() for k, v in layer.named_parameters()}
        tx, ta = x.detach().clone().requires_grad_(), a.detach().clone().requires_grad_()
        grad_legs("torch_layer", lambda: torch_layer(p16, tx, tab, mask, alpha), list(p16.values()) + [tx], dy, legs)
        grad_legs("torch_norm", lambda: rms(ta + alpha * tx, p16["norm1.weight"]), [ta, tx, p16["norm1.weight"]], dy, legs)

        def torch_gated():
            y, gate = torch.nn.functional.linear(tx, p16["ff.fc1.weight"]).chunk(2, dim=-1)
            return y * torch.nn.functional.silu(gate)

        grad_legs("torch_gated", torch_gated, [tx, p16["ff.fc1.weight"]], dh, legs)
    ms, reps, iters = timed(legs, seconds, repeats)
    res = {"N": N, "T": T, "d_model": D, "nhead": H, "dim_feedforward": F, "window": list(WINDOW), "repeats_ms": reps, "iters": iters}
    res.update({"ms_" + k: v for k, v in ms.items()})
    for part in ("layer", "norm", "gated") + (("torch_layer", "torch_norm", "torch_gated") if with_torch else ()):
        res["ms_%s_backward" % part] = ms[part + "_forward_backward"] - ms[part + "_forward"]
    res["norm_backward_gbytes_per_s"] = 5.0 * M * D * 2 / res["ms_norm_backward"] / 1e6
    res["norm_forward_gbytes_per_s"] = 3.0 * M * D * 2 / res["ms_norm_forward"] / 1e6
    res["gated_recompute_share"] = ms["gated_recompute_gemm"] / res["ms_gated_backward"]
    res["gated_saved_bytes_per_layer"] = M * 2 * F * 2
    if with_torch:
        for part in ("layer", "norm", "gated"):
            res["speedup_%s_forward_vs_torch" % part] = ms["torch_%s_forward" % part] / ms[part + "_forward"]
            res["speedup_%s_forward_backward_vs_torch" % part] = ms["torch_%s_forward_backward" % part] / ms[part + "_forward_backward"]
        legs["layer_forward_backward"]()
        legs["torch_layer_forward_backward"]()
        torch.cuda.synchronize()
        res["difference_vs_torch"] = {"y": rel(legs["layer_forward"](), legs["torch_layer_forward"]()), "dx": rel(x.grad, tx.grad),
                                      "dfc1": rel(layer.ff.fc1.weight.grad, p16["ff.fc1.weight"].grad),
                                      "dnorm2": rel(layer.norm2.weight.grad, p16["norm2.weight"].grad)}
    return res


def model_config():
    """The v5 `sup` stack (tests/golden/configs/dna_r10.4.1@v5.0.toml) with the batchnorm taken off the convolutions."""
    conv = lambda i, o, k, s: dict(type="convolution", insize=i, size=o, winlen=k, stride=s, padding=k // 2, bias=True, activation="swish")   # noqa: E731
    alpha, beta = deepnorm_params(DEPTH)
    layer = dict(type="transformerencoderlayer", d_model=D, nhead=H, dim_feedforward=F, deepnorm_alpha=alpha, deepnorm_beta=beta,
                 attn_window=list(WINDOW))
    encoder = {"type": "namedserial",
               "conv": {"type": "serial", "sublayers": [conv(1, 64, 5, 1), conv(64, 64, 5, 1), conv(64, 128, 9, 3), conv(128, 128, 9, 2),
                                                        conv(128, D, 5, 2), {"type": "permute", "dims": [0, 2, 1]}]},
               "transformer_encoder": {"type": "stack", "depth": DEPTH, "layer": layer},
               "upsample": {"type": "linearupsample", "d_model": D, "scale_factor": 2},
               "crf": {"type": "linearcrfencoder", "insize": D, "n_base": 4, "state_len": 5, "bias": False, "scale": 5.0, "blank_score": 2.0,
                       "expand_blanks": True, "permute": [1, 0, 2]}}
    return {"model": {"type": "seqdistmodel", "package": "bonito.transformer", "seqdist": {"state_len": 5, "alphabet": ["N", "A", "C", "G", "T"]},
                      "encoder": encoder}}


def bench_model(N, T, seconds, repeats, dev):
    from bonito_amd.transformer import Model
    torch.manual_seed(7)
    model = Model(model_config()).to(dev)
    L = 12 * T
    g = torch.Generator().manual_seed(45)
    x = torch.randn(N, 1, L, generator=g).half().to(dev)
    lengths = torch.randint(L // 24, L // 12, (N,), generator=g)
    targets = torch.randint(1, 5, (N, int(lengths.max())), generator=g)
    params = list(model.parameters())

    def forward():
        with torch.no_grad():
            model.forward_train(x)

    def step():
        for p in params:
            p.grad = None
        model.loss(model.forward_train(x), targets, lengths).backward()

    ms, reps, iters = timed({"forward_train": forward, "step": step}, seconds, repeats)
    return {"N": N, "samples": L, "T": T, "depth": DEPTH, "state_len": 5, "ms_forward_train": ms["forward_train"], "ms_step": ms["step"],
            "repeats_ms": reps, "iters": iters, "finite": all(bool(torch.isfinite(p.grad).all()) for p in params)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--N", default="16,64")
    ap.add_argument("--seconds", type=float, default=0.5, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transformer_train_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("transformer_train_bench: no HIP device; nothing is measured without one")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "seconds": args.seconds, "repeats": args.repeats, "shapes": []}

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")

    for N in (int(v) for v in args.N.split(",")):
        res["shapes"].append(bench_shape(N, args.T, args.seconds, args.repeats, not args.no_torch, dev))
        write()
        torch.cuda.empty_cache()
    if not args.no_model:
        res["model"] = bench_model(16, args.T, args.seconds, args.repeats, dev)
        write()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

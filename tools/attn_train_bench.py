#!/usr/bin/env python3
"""Time the training attention core (bonito_amd/csrc/attention_train.hip): the forward that keeps lse, and forward + backward, beside
torch's fp16 scaled_dot_product_attention under the band mask with its autograd on the same device - what the reference's
MultiHeadAttention falls back to without flash-attn, and the only thing a user could have called before.

    python tools/attn_train_bench.py [--T 2000 --H 8 --N 16,64 --window 127,128 --seconds 0.5 --repeats 5 --no-torch --out FILE]

Inputs are seeded: qkv ~ N(0, 0.7) fp16 [N][T][3][H][64], dout ~ N(0, 1) fp16. bh_attention_train_forward / _backward are called through the C
ABI with every buffer allocated once. Each leg is warmed up with one call, which also sizes the timed window: `iters` back-to-back calls
that take at least --seconds between two HIP events on the current stream; the figure is the MEDIAN over --repeats windows, and the legs
alternate (ours, torch, ours, ...) so that a drift of the shared host hits both. torch gets q and k rotated beforehand (the rotation is not
in its time) and the [T][T] boolean band mask; its output and gradients are compared with ours (largest difference over largest
element) - a timing of something that computes another function would say nothing.

Counted work (the algorithm's, from the shape alone): per (chunk, head, visible pair) the forward does 2 GEMMs of 2 x 64 flop (S, PV), the
backward recomputes S in both passes and does dP twice, dV, dQ, dK: 7 GEMMs - 3.5 x the forward's. `backward_over_forward` is the
measured ratio beside that 3.5. No time is fixed in advance: nobody has measured this before. The result is rewritten after every shape.
Prints one JSON line and writes it to --out (default profiles/attn_train_bench.json)."""
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

from bonito_amd import _lib  # noqa: E402


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
    """legs: {name: fn} -> {name: (median ms, all repeats, iters)}; the legs alternate inside every repeat."""
    iters = {k: window_iters(fn, seconds) for k, fn in legs.items()}
    out = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            out[k].append(one_window(fn, iters[k]))
    return {k: (statistics.median(v), v, iters[k]) for k, v in out.items()}


def rotary(x, tab):
    """x [N, T, H, 64] fp16, tab [T, 32, 2] fp32 -> rotated, fp16 (torch's leg gets q and k rotated outside its timed region)."""
    cos, sin = tab[None, :, None, :, 0], tab[None, :, None, :, 1]
    x1, x2 = x[..., :32].float(), x[..., 32:].float()
    return torch.cat([x1 * cos - x2 * sin, x1 * sin + x2 * cos], dim=-1).half()


def rel(a, b):
    return float((a.float() - b.float()).abs().max() / b.float().abs().max())


def bench_shape(N, T, H, win, seconds, repeats, with_torch, dev):
    g = torch.Generator(device=dev).manual_seed(41)
    qkv = torch.empty((N, T, 3, H, 64), dtype=torch.float32, device=dev).normal_(0.0, 0.7, generator=g).half()
    dout = torch.empty((N, T, H * 64), dtype=torch.float32, device=dev).normal_(generator=g).half()
    lib, st = _lib.lib(), _lib.stream_ptr(dev)
    tab_h = np.empty((T, 32, 2), np.float32)
    _lib.check(lib.bh_rotary_table(T, 64, tab_h.ctypes.data), "bh_rotary_table")
    tab = torch.from_numpy(tab_h).to(dev)
    sb, wb = lib.bh_attention_train_saved_bytes(N, T, H), lib.bh_attention_train_backward_workspace(N, T, H, win[0], win[1])
    if sb == 0 or wb == 0:
        raise SystemExit("attn_train_bench: shape N=%d T=%d H=%d window %s is not served" % (N, T, H, win))
    out, dqkv = torch.empty_like(dout), torch.empty_like(qkv)
    saved = torch.empty(sb, dtype=torch.uint8, device=dev)
    ws = torch.empty(wb, dtype=torch.uint8, device=dev)

    def forward():
        _lib.check(lib.bh_attention_train_forward(_lib.ptr(qkv), _lib.ptr(tab), N, T, H, 64, win[0], win[1], _lib.ptr(out), _lib.ptr(saved), sb, st),
                   "bh_attention_train_forward")

    def both():
        forward()
        _lib.check(lib.bh_attention_train_backward(_lib.ptr(qkv), _lib.ptr(tab), _lib.ptr(out), _lib.ptr(saved), _lib.ptr(dout), N, T, H, 64,
                                                   win[0], win[1], _lib.ptr(dqkv), _lib.ptr(ws), wb, st), "bh_attention_train_backward")

    out_inf = torch.empty_like(dout)

    def forward_inference():          # bh_attention: the same kernel without lse, what the engine launches for windows the ring kernels do not serve
        _lib.check(lib.bh_attention(_lib.ptr(qkv), _lib.ptr(out_inf), _lib.ptr(tab), N, T, H, 64, win[0], win[1], st), "bh_attention")

    legs = {"forward": forward, "forward_inference": forward_inference, "forward_backward": both}
    res = {"N": N, "T": T, "H": H, "window": list(win), "saved_bytes": int(sb), "workspace_bytes": int(wb)}
    if with_torch:
        q, k = rotary(qkv[:, :, 0], tab), rotary(qkv[:, :, 1], tab)
        tq, tk, tv = (t.permute(0, 2, 1, 3).contiguous() for t in (q, k, qkv[:, :, 2]))       # [N, H, T, 64]
        i = torch.arange(T, device=dev)
        mask = (i[None, :] >= i[:, None] - win[0]) & (i[None, :] <= i[:, None] + win[1])
        leaves = [t.clone().requires_grad_() for t in (tq, tk, tv)]
        tdo = dout.view(N, T, H, 64).permute(0, 2, 1, 3).contiguous()
        sdpa = torch.nn.functional.scaled_dot_product_attention

        def torch_forward():
            with torch.no_grad():
                return sdpa(tq, tk, tv, attn_mask=mask)

        def torch_both():
            for t in leaves:
                t.grad = None
            sdpa(*leaves, attn_mask=mask).backward(tdo)

        legs.update({"torch_forward": torch_forward, "torch_forward_backward": torch_both})
    t = timed(legs, seconds, repeats)
    for name, (ms, reps, iters) in t.items():
        res["ms_" + name] = ms
        res.setdefault("repeats_ms", {})[name] = reps
        res.setdefault("iters", {})[name] = iters
    res["ms_backward"] = res["ms_forward_backward"] - res["ms_forward"]
    res["backward_over_forward"] = res["ms_backward"] / res["ms_forward"]
    res["backward_over_forward_counted"] = 3.5
    res["finite"] = bool(torch.isfinite(dqkv).all()) and bool(torch.isfinite(out).all())
    # visible (query, key) pairs of one (chunk, head), from the window alone
    ii = np.arange(T)
    pairs = int((np.minimum(ii + win[1], T - 1) - np.maximum(ii - win[0], 0) + 1).sum())
    flop_f = 2.0 * 2 * 64 * pairs * N * H
    res["visible_pairs"] = pairs
    res["tflops_forward"] = flop_f / res["ms_forward"] / 1e9
    res["tflops_backward"] = 3.5 * flop_f / res["ms_backward"] / 1e9
    if with_torch:
        res["ms_torch_backward"] = res["ms_torch_forward_backward"] - res["ms_torch_forward"]
        res["torch_backward_over_forward"] = res["ms_torch_backward"] / res["ms_torch_forward"]
        res["speedup_forward_vs_torch"] = res["ms_torch_forward"] / res["ms_forward"]
        res["speedup_forward_backward_vs_torch"] = res["ms_torch_forward_backward"] / res["ms_forward_backward"]
        both()
        torch_both()
        torch.cuda.synchronize()
        want = torch_forward().permute(0, 2, 1, 3).reshape(N, T, H * 64)
        # torch differentiates with respect to the ROTATED q and k, so ours are rotated forward for the comparison: dq = rot^-1(dq~) / 8
        # gives rot(dq) = dq~ / 8, torch's gradient of rot(q) (its own 1/8 sits inside the scores); rot(dk) = dk~ likewise
        res["difference_vs_torch"] = {"out": rel(out, want),
                                      "dq": rel(rotary(dqkv[:, :, 0], tab), leaves[0].grad.permute(0, 2, 1, 3)),
                                      "dk": rel(rotary(dqkv[:, :, 1], tab), leaves[1].grad.permute(0, 2, 1, 3)),
                                      "dv": rel(dqkv[:, :, 2], leaves[2].grad.permute(0, 2, 1, 3))}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=2000)
    ap.add_argument("--H", type=int, default=8)
    ap.add_argument("--N", default="16,64")
    ap.add_argument("--window", default="127,128")
    ap.add_argument("--seconds", type=float, default=0.5, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_train_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("attn_train_bench: no HIP device; nothing is measured without one")
    dev = torch.device("cuda:0")
    win = tuple(int(v) for v in args.window.split(","))
    res = {"device": torch.cuda.get_device_name(0), "seconds": args.seconds, "repeats": args.repeats, "shapes": []}
    for N in (int(v) for v in args.N.split(",")):
        res["shapes"].append(bench_shape(N, args.T, args.H, win, args.seconds, args.repeats, not args.no_torch, dev))
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

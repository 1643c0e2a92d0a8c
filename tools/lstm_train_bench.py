#!/usr/bin/env python3
"""Time one training LSTM layer (bonito_amd/csrc/lstm_train.hip): the forward that keeps the gates, and forward + backward, beside the
half-precision torch.nn.LSTM on the same device - the only thing a user could have called before it.

    python tools/lstm_train_bench.py [--T 600 --N 64,512,2048 --H 96,384,1024 --window 0.3 --repeats 3 --no-torch --out FILE]

Inputs are seeded: x ~ N(0, 1) fp16 [T][N][H], weights uniform in +-1/sqrt(H) (fp32 on the device, as the entry points take them), a
bias, dh ~ N(0, 1) fp16. bh_lstm_train_forward / bh_lstm_train_backward are called through the C ABI with every buffer allocated once.
Each shape is warmed up with one call, which also sizes the timed window: `iters` back-to-back calls that take at least --window seconds
between two HIP events on the current stream; the figure is the MEDIAN over --repeats windows. torch.nn.LSTM(H, H).half() runs the same
x and dh (forward under no_grad; forward + backward with gradients for x and its parameters); where it does not run, the error is
recorded and the shape goes on (a device fault ends the run); it is not started at all where its gate tensor [T][N][4H] reaches 2^31
bytes (TORCH_LIMIT_BYTES). No threshold is set: nobody has measured this before. `workgroups` is how many workgroups the two recurrent
kernels occupy (one per tile of 16 chunks; the device has 256 CUs). The result is rewritten after every shape, so a run that
is cut short leaves what it measured. Prints one JSON line and writes it to --out (default profiles/lstm_train_bench.json)."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bonito_amd import _lib  # noqa: E402

# torch.nn.LSTM(384, 384).half() at T = 600, N = 2048 (a gate tensor [T][N][4H] of 3.8e9 bytes) ended in an illegal memory access inside
# torch's own backend on the MI355X, after this project's calls on the same shape had completed and been read back; the three smaller
# shapes with the same N or the same H ran. The cause is not known (a 32-bit byte offset is a guess), so torch is not run from 2^31
# bytes on, and the shape is reported as skipped
TORCH_LIMIT_BYTES = 1 << 31


def timed(fn, window, repeats):
    """-> (median ms per call, all repeats, iters). One warm-up call, timed on its own, sizes the window."""
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
    return statistics.median(out), out, iters


def bench_shape(T, N, H, window, repeats, with_torch, dev):
    g = torch.Generator(device=dev).manual_seed(31)
    k = 1.0 / math.sqrt(H)
    x = torch.empty((T, N, H), dtype=torch.float32, device=dev).normal_(generator=g).half()
    dh = torch.empty((T, N, H), dtype=torch.float32, device=dev).normal_(generator=g).half()
    w_ih = (torch.rand((4 * H, H), device=dev, generator=g) * 2 - 1) * k
    w_hh = (torch.rand((4 * H, H), device=dev, generator=g) * 2 - 1) * k
    bias = torch.empty(4 * H, device=dev).normal_(0.0, 0.3, generator=g)
    lib, st = _lib.lib(), _lib.stream_ptr(dev)
    sb, wb = lib.bh_lstm_train_saved_bytes(T, N, H), lib.bh_lstm_train_backward_workspace(T, N, H)
    h, dx = torch.empty_like(x), torch.empty_like(x)
    saved = torch.empty(sb, dtype=torch.uint8, device=dev)
    ws = torch.empty(wb, dtype=torch.uint8, device=dev)
    dwi, dwh = torch.empty_like(w_ih), torch.empty_like(w_hh)
    db = torch.empty_like(bias)

    def forward():
        _lib.check(lib.bh_lstm_train_forward(_lib.ptr(x), _lib.ptr(w_ih), _lib.ptr(w_hh), _lib.ptr(bias), T, N, H, 0, _lib.ptr(h),
                                             _lib.ptr(saved), sb, st), "bh_lstm_train_forward")

    def backward():
        _lib.check(lib.bh_lstm_train_backward(_lib.ptr(x), _lib.ptr(w_ih), _lib.ptr(w_hh), _lib.ptr(h), _lib.ptr(saved), _lib.ptr(dh), T, N, H, 0,
                                              _lib.ptr(dx), _lib.ptr(dwi), _lib.ptr(dwh), _lib.ptr(db), _lib.ptr(ws), wb, st),
                   "bh_lstm_train_backward")

    def both():
        forward()
        backward()

    res = {"T": T, "N": N, "H": H, "workgroups": int(lib.bh_lstm_train_workgroups(N)), "saved_bytes": int(sb), "workspace_bytes": int(wb)}
    ms_f, all_f, it_f = timed(forward, window, repeats)
    ms_b, all_b, it_b = timed(both, window, repeats)
    res.update({"ms_forward": ms_f, "ms_forward_backward": ms_b, "iters": [it_f, it_b], "repeats_ms": {"forward": all_f, "forward_backward": all_b},
                "finite": bool(torch.isfinite(dx).all()) and bool(torch.isfinite(dwh).all())})
    # the algorithm's operations: 2 x 4H x 2H per row and pass for the forward, twice that again for the backward (dx and d_t, dW)
    flop_f = 2.0 * T * N * 4 * H * 2 * H
    res["tflops_forward"] = flop_f / ms_f / 1e9
    res["tflops_forward_backward"] = 3.0 * flop_f / ms_b / 1e9
    if with_torch and T * N * 4 * H * 2 >= TORCH_LIMIT_BYTES:
        res["torch_skipped"] = "gate tensor of %d bytes: torch.nn.LSTM half is not run from 2^31 bytes on (see the module docstring)" % (T * N * 4 * H * 2)
    elif with_torch:
        try:
            m = torch.nn.LSTM(H, H).to(dev).half()
            with torch.no_grad():
                m.weight_ih_l0.copy_(w_ih)
                m.weight_hh_l0.copy_(w_hh)
                m.bias_ih_l0.copy_(bias)
                m.bias_hh_l0.zero_()
            xt = x.clone().requires_grad_(True)

            def torch_forward():
                with torch.no_grad():
                    return m(x)[0]

            def torch_both():
                xt.grad = None
                m.zero_grad(set_to_none=True)
                m(xt)[0].backward(dh)

            ms_tf, all_tf, _ = timed(torch_forward, window, repeats)
            ms_tb, all_tb, _ = timed(torch_both, window, repeats)
            res.update({"ms_torch_forward": ms_tf, "ms_torch_forward_backward": ms_tb,
                        "repeats_ms_torch": {"forward": all_tf, "forward_backward": all_tb},
                        "max_abs_difference_h_vs_torch": float((torch_forward().float() - h.float()).abs().max())})
        except Exception as exc:                                            # recorded, and the shape goes on ...
            res["torch_error"] = "%s: %s" % (type(exc).__name__, str(exc)[:300])
            res["device_fault"] = "HIP error" in str(exc)                   # ... unless the device faulted: main() stops there
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=600)
    ap.add_argument("--N", default="64,512,2048")
    ap.add_argument("--H", default="96,384,1024")
    ap.add_argument("--window", type=float, default=0.3, help="seconds of back-to-back calls per timed window")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstm_train_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lstm_train_bench: no HIP device; nothing is measured without one")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "window_s": args.window, "repeats": args.repeats, "direction": "forward in time",
           "shapes": []}
    for H in (int(v) for v in args.H.split(",")):
        for N in (int(v) for v in args.N.split(",")):
            res["shapes"].append(bench_shape(args.T, N, H, args.window, args.repeats, not args.no_torch, dev))
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "w") as fh:
                    fh.write(json.dumps(res) + "\n")
            if res["shapes"][-1].get("device_fault"):
                print(json.dumps(res))
                raise SystemExit("lstm_train_bench: the device faulted in torch.nn.LSTM at N=%d H=%d; nothing more is started" % (N, H))
            torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

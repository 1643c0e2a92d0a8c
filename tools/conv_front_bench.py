#!/usr/bin/env python3
"""The fused front end (bh_conv1d_front3) alone at the hac model's layer shapes: conv1 1 -> 16 (5 taps), conv2 16 -> 16 (5 taps),
conv3 16 -> 384 (19 taps, stride 6), swish and the models' clamp (-0.5, 3.5) behind each, time-major output as the recurrent stack
reads it. HIP events around single launches, warm-up first, median / minimum of the timed ones.

    python tools/conv_front_bench.py                                   # 512 x 10000 and 2048 x 10000
    python tools/conv_front_bench.py --set conv_front_pipe=0           # the kernel without the conv1/conv2 | conv3 pipeline
    python tools/conv_front_bench.py --set conv_front_wgs=128 --batches 2048
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from bonito_amd import _lib, decode

K1, K2, K3, S3, COUT = 5, 5, 19, 6, 384
LO, HI = -0.5, 3.5


def pack(lib, w, cin, cout, k):
    pk = np.zeros(lib.bh_conv1d_packed_halves(cin, cout, k), np.uint16)
    _lib.check(lib.bh_conv1d_pack(w.ctypes.data_as(C.c_void_p), cin, cout, k, pk.ctypes.data_as(C.c_void_p)), "bh_conv1d_pack")
    return torch.from_numpy(pk.view(np.int16)).cuda()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", default="512,2048", help="comma-separated chunk counts per launch")
    ap.add_argument("--chunk", type=int, default=10000)
    ap.add_argument("--launches", type=int, default=30, help="timed launches per shape (>= 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--set", action="append", default=[], metavar="NAME=VALUE", help="process-wide option, e.g. conv_front_pipe=0")
    a = ap.parse_args()
    assert a.launches >= 20
    lib = _lib.lib()
    opts = {}
    for s in a.set:
        k, v = s.split("=")
        decode.set_option(k, int(v))
        opts[k] = int(v)
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    w1 = torch.from_numpy((rng.standard_normal((16, K1)) * 0.4).astype(np.float32)).cuda()
    b1 = torch.from_numpy((rng.standard_normal(16) * 0.1).astype(np.float32)).cuda()
    w2 = pack(lib, (rng.standard_normal((16, 16, K2)) * 0.15).astype(np.float32), 16, 16, K2)
    b2 = torch.from_numpy((rng.standard_normal(16) * 0.1).astype(np.float32)).cuda()
    w3 = pack(lib, (rng.standard_normal((COUT, 16, K3)) * 0.08).astype(np.float32), 16, COUT, K3)
    b3 = torch.from_numpy((rng.standard_normal(COUT) * 0.1).astype(np.float32)).cuda()
    p = _lib.ptr
    for N in (int(v) for v in a.batches.split(",")):
        L0 = a.chunk
        L3 = (L0 + 2 * (K3 // 2) - K3) // S3 + 1
        sig = torch.randn(N, L0, device="cuda").half()
        out = torch.empty(L3 * N * COUT, device="cuda", dtype=torch.half)

        def launch():
            _lib.check(lib.bh_conv1d_front3(p(sig), N, L0, p(w1), p(b1), K1, K1 // 2, 1, LO, HI, p(w2), p(b2), K2, K2 // 2, 1, LO, HI,
                                            p(w3), p(b3), COUT, K3, S3, K3 // 2, 1, LO, HI, p(out), COUT, N * COUT, _lib.stream_ptr()),
                       "bh_conv1d_front3")

        for _ in range(a.warmup):
            launch()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        print(json.dumps({"tool": "conv_front_bench", "N": N, "L0": L0, "L3": L3, "options": opts, "kernel": lib.bh_conv1d_last_kernel(),
                          "launches": a.launches, "median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
                          "max_ms": round(max(ms), 4), "out_GBps": round(out.numel() * 2 / statistics.median(ms) / 1e6, 1),
                          "checksum": float(out.float().sum().item())}))


if __name__ == "__main__":
    main()

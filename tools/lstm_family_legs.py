#!/usr/bin/env python3
"""One round of the per-family timing legs of profiles/lstm_ring_parent_vs_branch.txt with the library BONITO_HIP_LIB names (default: the
tree's): the encoder forward of a five-layer LSTM-CRF model of the family's width at its product shape, HIP events around each call, the
median of six calls behind three warm-up calls -> one JSON line. Two libraries are compared by alternating processes:

    for i in 1 2 3 4 5; do BONITO_HIP_LIB=parent/libbonito_hip.so python tools/lstm_family_legs.py; python tools/lstm_family_legs.py; done

The convolutions and the CRF head are inside the timed call (a few percent of it at these shapes); where both libraries were built from the
same sources but for lstm.hip / lstm_q8.hip a difference is the recurrent kernels', but the spread of a leg includes theirs."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from bonito_amd import nn as bnn, synthetic
from bonito_amd.engine import HipEncoder

LEGS = [  # name, H, N, L, quantize, options, kernel expected in describe()
    ("wgx2_384_1024x1667", 384, 1024, 10002, False, {}, "lstm_layer_wgx2_kernel<12,3>"),
    ("wgx_384_512x1667", 384, 512, 10002, False, {}, "lstm_layer_wgx_kernel<12,3>"),
    ("cta_96_512x1667", 96, 512, 10002, False, {}, "lstm_layer_cta_kernel"),
    ("wide_1024_256x3334", 1024, 256, 20004, False, {}, "lstm_layer_wide_kernel"),
    ("fused_384_512x1667", 384, 512, 10002, False, {"lstm_exchange": 0}, "lstm_layer_fused_kernel"),
    ("stream_768_128x1667", 768, 128, 10002, False, {"lstm_wide": 0}, "lstm_layer_kernel"),
    ("q8_384_512x1667", 384, 512, 10002, True, {}, "lstm_layer_q8_kernel"),
]
out = {"lib": os.environ.get("BONITO_HIP_LIB", "tree")}
for name, H, N, L, quantize, options, kernel in LEGS:
    torch.manual_seed(1)
    model = bnn.from_dict(synthetic.lstm_crf_encoder_config(H, 3, n_lstm=5)).eval()
    x = torch.randn(N, 1, L, generator=torch.Generator().manual_seed(2)).half().cuda()
    enc = HipEncoder(model, batchsize=N, chunksize=L, quantize=quantize)
    for k, v in options.items():
        enc.set_option(k, v)
    for _ in range(3):
        enc(x)
    torch.cuda.synchronize()
    assert kernel in enc.describe(), (name, enc.describe())
    ts = []
    for _ in range(6):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); enc(x); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    enc.check()
    enc.close()
    del enc, model, x
    torch.cuda.empty_cache()
    ts.sort()
    out[name] = round((ts[2] + ts[3]) / 2, 4)
print(json.dumps(out), flush=True)

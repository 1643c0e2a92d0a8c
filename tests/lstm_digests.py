"""The cases and the sha256 digests that pin the recurrent inference kernels (csrc/lstm.hip, csrc/lstm_q8.hip) to the bytes of the commit
before their shared parts moved into csrc/lstm_ring.h. tools/lstm_kernel_digests.py writes tests/golden/lstm_kernels_parent.json from a
build of that commit; tests/test_gpu_lstm.py and tests/test_gpu_q8.py recompute the digests with the tree's library and compare. The kernels
have no atomics in their arithmetic and no order that depends on scheduling, so the bytes do not depend on the machine.

Cases, the smallest that reach each block the kernels used to carry a copy of (inputs: lstm_ref.make_case "typical" / q8_ref.typical_case,
seed SEED; T = 5 covers the first re-arm at step 2 and the slot wrap at step 4):
  a  every (family, H) instance at T = 5, two rings, forward and reverse;
  b  one H per family at T = 1, 2, 3 (the prologue's special cases), 11 and 14 (one and two unrolled blocks of wgx2's fast path);
  c  wgx2 at three rings (a lone ring on the `two == false` path);
  d  the write-through policy, and through the engine (the only door for "lstm_tune") the bit-5 spread for wgx, wgx2, wide and q8 and the
     generic section code (bit 6) of wgx2 at 384;
  e  the wide kernel with the hand-off through the output tensor ("lstm_exchange" 0: flags bit 1)."""
import ctypes as C
import hashlib
import math

import numpy as np
import torch

import lstm_ref as lr
import q8_ref
from bonito_amd import _lib

SEED = 7
WIDTHS = {"wave": [32 * k for k in range(1, 17)], "fused": [32 * k for k in range(1, 17)], "stream": [64 * k for k in range(1, 17)],
          "wgx": [96, 192, 288, 384, 64, 128, 256], "wgx2": [96, 192, 288, 384, 64, 128, 256], "cta": [64, 96, 128],
          "wide": [640, 768, 896, 1024]}                 # family -> every width with an instance (tests/test_gpu_lstm.py reads these three)
MAIN = {"wave": 384, "fused": 384, "wgx": 384, "wgx2": 384, "cta": 96, "wide": 1024, "stream": 1024}
HAS_POLICY = ("wave", "fused", "stream", "wgx", "wgx2", "wide")      # (cta exchanges through LDS only)


def sha(t):
    if isinstance(t, torch.Tensor):
        t = t.contiguous().view(torch.uint8).flatten().cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(t).tobytes()).hexdigest()


def fp16_cases(family):
    """-> [(H, T, rings, reverse, flags)]"""
    out = [(H, 5, 2, rev, 0) for H in WIDTHS[family] for rev in (0, 1)]                               # a
    out += [(MAIN[family], T, 2, T % 2, 0) for T in (1, 2, 3, 11, 14)]                                # b
    if family == "wgx2":
        out += [(H, 11, 3, rev, 0) for H in (384, 96) for rev in (0, 1)]                              # c
    if family in HAS_POLICY:
        out += [(MAIN[family], 11, 2, rev, 1) for rev in (0, 1)]                                      # d: write-through
    if family == "wide":
        out += [(H, 5, 2, rev, flags) for H in WIDTHS["wide"] for rev, flags in ((0, 2), (1, 3))]     # e
        out += [(1024, 11, 2, 0, 2)]
    return out


def fp16_digest(family, H, T, rings, reverse, flags):
    N = rings * (32 if family == "wide" else 16)
    x, w_ih, w_hh, bias = lr.make_case("typical", T, N, H, seed=SEED)
    xd = x.cuda()
    out = torch.zeros(T, N, H, dtype=torch.int16, device="cuda")
    w1, w2, b = (np.ascontiguousarray(a.numpy(), np.float32) for a in (w_ih, w_hh, bias))
    rc = _lib.lib().bh_lstm_layer_family(_lib.ptr(xd), w1.ctypes.data_as(C.c_void_p), w2.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p),
                                         T, N, H, reverse, _lib.LSTM_FAMILIES[family], flags, _lib.ptr(out), _lib.stream_ptr())
    _lib.check(rc, "bh_lstm_layer_family(%s, H=%d, T=%d, N=%d, flags=%d)" % (family, H, T, N, flags))
    torch.cuda.synchronize()
    return sha(out)


def fp16_key(H, T, rings, reverse, flags):
    return "H%d-T%d-R%d-%s-f%d" % (H, T, rings, "rev" if reverse else "fwd", flags)


def q8_cases():
    """-> [(H, variant, T, reverse)]"""
    out = [(H, v, 5, rev) for H, v in sorted(q8_ref.INSTANCES) for rev in (0, 1)]                     # a
    out += [(384, 0, T, T % 2) for T in (1, 2, 3, 11, 14)]                                            # b
    return out


def q8_digest(H, variant, T, reverse):
    """The three instances of the hook (sums given / h16 without sums / fragments only): every output buffer of each."""
    N = 32
    x, w_ih, w_hh, bias = q8_ref.typical_case(H, T, N, 1.0, seed=SEED)
    xd = torch.as_tensor(x).cuda()
    got = {}
    for mode in ("dbg", "last", "inner"):
        h16 = torch.full((T, N, H), -1, dtype=torch.int16, device="cuda")
        hq = torch.full((T * (N // 16) * q8_ref.nk8(H) * 1024,), -128, dtype=torch.int8, device="cuda")
        sums = torch.zeros(T, N, 4 * H, 2, dtype=torch.int32, device="cuda") if mode == "dbg" else None
        rc = _lib.lib().bh_lstm_q8_layer(_lib.ptr(xd), 1.0, w_ih.ctypes.data_as(C.c_void_p), w_hh.ctypes.data_as(C.c_void_p),
                                         bias.ctypes.data_as(C.c_void_p), T, N, H, reverse, variant, _lib.ptr(h16) if mode != "inner" else None,
                                         _lib.ptr(hq), _lib.ptr(sums) if sums is not None else None, _lib.stream_ptr())
        _lib.check(rc, "bh_lstm_q8_layer(H=%d, variant=%d, T=%d, %s)" % (H, variant, T, mode))
        torch.cuda.synchronize()
        got[mode] = {"h16": sha(h16), "hq": sha(hq)}
        if sums is not None:
            got[mode]["sums"] = sha(sums)
    return got


def q8_key(H, variant, T, reverse):
    return "H%d-v%d-T%d-%s" % (H, variant, T, "rev" if reverse else "fwd")


# d, the part only the engine reaches: name -> (H, batch, quantize, option, value); two recurrent layers (one per direction), 11 time steps.
# 544 chunks = 34 rings at H = 384: more than a launch of single rings holds, so the layer runs the paired kernel.
ENGINE_CASES = {"wgx-384-spread": (384, 32, False, "lstm_tune", 32), "wgx2-384-spread": (384, 544, False, "lstm_tune", 32),
                "wgx2-384-generic": (384, 544, False, "lstm_tune", 64), "wide-1024-spread": (1024, 64, False, "lstm_tune", 32),
                "q8-384-spread": (384, 32, True, "lstm_tune", 32), "q8-384-write-through": (384, 32, True, "lstm_force_slow", 1)}
ENGINE_KERNEL = {"wgx": "lstm_layer_wgx_kernel", "wgx2": "lstm_layer_wgx2_kernel", "wide": "lstm_layer_wide_kernel", "q8": "lstm_layer_q8_kernel"}


def engine_digest(name):
    """sha256 of the scores of a whole encoder (convolutions, two recurrent layers, linear layer, CRF head) on a model of bnn.from_dict: it
    pins the recurrent kernels only while those other units and the model builder stand still; after a change to them on purpose the golden
    is rewritten from the commit before that change."""
    from bonito_amd import nn as bnn, synthetic
    from bonito_amd.engine import HipEncoder
    H, N, quantize, option, value = ENGINE_CASES[name]
    torch.manual_seed(SEED)
    model = bnn.from_dict(synthetic.lstm_crf_encoder_config(H, 3, n_lstm=2)).eval()
    g = torch.Generator().manual_seed(SEED)
    with torch.no_grad():          # the matrices from an explicit generator: torch's own initialisation of a large tensor depends on the thread count
        for _, p in sorted(model.named_parameters()):
            if p.dim() >= 2:
                p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) / math.sqrt(p.numel() // p.shape[0]))
    x = torch.randn(N, 1, 66, generator=torch.Generator().manual_seed(SEED)).half().cuda()
    enc = HipEncoder(model, batchsize=N, chunksize=66, quantize=quantize)
    enc.set_option(option, value)
    out = enc(x).clone()
    enc.check()
    assert ENGINE_KERNEL[name.split("-")[0]] + "<" in enc.describe(), enc.describe()
    enc.close()
    return sha(out)

#!/usr/bin/env python3
"""sha256 of what the block attention kernels write, one case per rung of their ladder: tests/golden/attention_block_parent.json.

    python tools/attn_block_digests.py LIBRARY [--out FILE]

LIBRARY is the libbonito_hip.so to pin, loaded in place of the tree's own. The committed file was written once on an MI355X against a build
of the commit BEFORE the kernels moved onto csrc/attn_block.h; tests/test_gpu_attention_train.py recomputes the digests with the tree's
library and compares. Inputs are those of that test (tests/attention_train_ref.make_case, kind gauss, seed 1). Per case: `out` and `saved`
(lse, the N*T*H fp32 words) of bh_attention_train_forward, `out` of bh_attention, `dqkv` of bh_attention_train_backward. The kernels use no
atomics and no order that depends on scheduling, so the bytes do not depend on the machine."""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((2, 130, 3, (3, 5)),           # 3 tiles: rung 6          (N, T, H, window); every T ends in a partial block of 128
         (2, 130, 3, (40, 41)),         # 7 tiles: rung 10
         (1, 300, 1, (127, 128)),       # 17 tiles: rung 18
         (1, 450, 1, (200, 200)),       # 26 tiles: rung 26
         (1, 17, 1, (0, 0)))            # a single visible key


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("library")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "attention_block_parent.json"))
    args = ap.parse_args()
    os.environ["BONITO_HIP_LIB"] = os.path.abspath(args.library)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import torch
    import attention_train_ref as tr
    from bonito_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("attn_block_digests: no HIP device")
    lib, st = _lib.lib(), _lib.stream_ptr()

    def sha(t, nbytes=None):
        raw = t.contiguous().view(torch.uint8).flatten().cpu().numpy().tobytes()
        return hashlib.sha256(raw if nbytes is None else raw[:nbytes]).hexdigest()

    cases = []
    for N, T, H, (wl, wr) in CASES:
        qkv, dout = (torch.from_numpy(a).cuda() for a in tr.make_case(N, T, H, "gauss", seed=1))
        tab_h = np.empty((T, 32, 2), np.float32)
        _lib.check(lib.bh_rotary_table(T, 64, tab_h.ctypes.data_as(C.c_void_p)), "bh_rotary_table")
        tab = torch.from_numpy(tab_h).cuda()
        sb, wb = lib.bh_attention_train_saved_bytes(N, T, H), lib.bh_attention_train_backward_workspace(N, T, H, wl, wr)
        assert sb > 0 and wb > 0, (N, T, H, wl, wr)
        out, out_inf, dqkv = torch.zeros_like(dout), torch.zeros_like(dout), torch.zeros_like(qkv)
        saved, ws = (torch.zeros(b, dtype=torch.uint8, device="cuda") for b in (sb, wb))
        _lib.check(lib.bh_attention_train_forward(_lib.ptr(qkv), _lib.ptr(tab), N, T, H, 64, wl, wr, _lib.ptr(out), _lib.ptr(saved), sb, st), "forward")
        _lib.check(lib.bh_attention(_lib.ptr(qkv), _lib.ptr(out_inf), _lib.ptr(tab), N, T, H, 64, wl, wr, st), "bh_attention")
        _lib.check(lib.bh_attention_train_backward(_lib.ptr(qkv), _lib.ptr(tab), _lib.ptr(out), _lib.ptr(saved), _lib.ptr(dout), N, T, H, 64, wl, wr,
                                                   _lib.ptr(dqkv), _lib.ptr(ws), wb, st), "backward")
        torch.cuda.synchronize()
        cases.append({"N": N, "T": T, "H": H, "window": [wl, wr], "train_out": sha(out), "saved": sha(saved, N * T * H * 4),
                      "inference_out": sha(out_inf), "dqkv": sha(dqkv)})
    text = json.dumps({"kind": "gauss", "seed": 1, "cases": cases}, indent=1) + "\n"
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()

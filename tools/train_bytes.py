#!/usr/bin/env python3
"""sha256 of what the training layers compute on a few small, seeded cases: the record that a change of the code left every byte alone.

    python tools/train_bytes.py [--out FILE]

Only the public functions of bonito_amd.rnn and bonito_amd.train_ops and the models' forward_train are called, so the same file runs in a checkout of an earlier
commit; run it there and here on the same device and compare the two lines (hashes of device output depend on the toolchain and are
not a committed golden). Inputs come from the generators of the tests (tests/lstm_ref.py, tests/lstm_train_ref.py,
tests/train_layers_ref.py; fixed seeds).

    LSTM (T, N, H, direction)   several blocks of rows with a short last one, T N % 32 != 0, a padded batch tile, T = 1 (no h_prev row
                                exists), both directions; h, dx, dw_ih, dw_hh, db with a bias gradient and dx, dw_ih, dw_hh without
    convolution                 CONV_CASES rows 0, 3, 4, 7, clamp on and off: y, dx, dw, db
    linear                      LINEAR_CASES rows 1, 3, 4, both row maps: y, dx, dw, db
    norm (M, D)                 the DeepNorm residual RMSNorm (tests/transformer_train_ref.py): a tail of rows, a second vector per lane, more
                                than one dw block; out, da, dx, dw
    gated (M, D, F)             fc1 + SwiGLU: h, dx, dw
    batchnorm (N, L, C, pad)    batch-statistics BatchNorm behind a convolution (tests/batchnorm_train_ref.py), swish: one block of rows and
                                several with a short last one, 65 vectors per row, zero-padded channels, clamp on and off, the time-major
                                store; y, mean, rstd, running_mean, running_var, dz, dgamma, dbeta
    model                       forward_train of the four small models of the model tests (the LSTM family with fused clamps and a linear
                                layer, the transformer family, the LSTM family with norm="batch", QuartzNet with dropout 0.1 and a fixed
                                seed), seeded weights, that test's batch, a seeded fp16 upstream gradient: the scores, every parameter's
                                .grad and every BatchNorm buffer

Prints one JSON line {case: {tensor: sha256}}."""
import argparse
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lstm_ref as lr  # noqa: E402
import lstm_train_ref as tr  # noqa: E402
import train_layers_ref as tl  # noqa: E402
from bonito_amd import rnn, train_ops  # noqa: E402

LSTM_CASES = ((150, 20, 64, False), (600, 5, 32, False), (37, 5, 32, True), (3, 37, 128, True), (1, 5, 32, False), (1, 5, 32, True),
              (24, 16, 384, False))
CONV_ROWS = (0, 3, 4, 7)
LINEAR_ROWS = (1, 3, 4)
NORM_CASES = ((5, 64), (257, 520), (130, 1024))          # (M, D)
NORM_ALPHA = 2.4494897
GATED_CASES = ((17, 64, 72), (1030, 128, 256), (33, 512, 2048))      # (M, D, F)
BATCHNORM_CASES = ((3, 5, 16, 4), (2, 257, 64, 0), (5, 1000, 520, 0))       # (N, L, C, zero-padded channels)


def sha(t):
    return None if t is None else hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def model_cases():
    """-> (name, model with seeded weights, x, the keywords of forward_train): the four small configurations of the model tests, each on
    that test's batch."""
    import batchnorm_train_ref as bn
    import conftest
    import test_gpu_quartznet_train_model as tq
    import test_gpu_train_model as tm
    import transformer_train_ref as tt
    from bonito_amd.crf.model import Model
    from bonito_amd.ctc import Model as CtcModel
    from bonito_amd.transformer import Model as TransformerModel
    for name, make, x, kwargs in (
            ("model lstm", lambda: Model(tm._new_config()), tm._batch(3)[0], {}),
            ("model transformer", lambda: TransformerModel(tt.model_config()), tt.model_batch(3)[0], {}),
            ("model lstm norm=batch", lambda: Model(bn.lstm_config()), tm._batch(3)[0], {"norm": "batch"}),
            ("model quartznet dropout=0.1", lambda: CtcModel(tq._config(0.1)), conftest.load_ctc_fixture()[2].half(),
             {"norm": "batch", "seed": tq.SEED})):
        torch.manual_seed(7)
        yield name, make(), x, kwargs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_bytes: no HIP device; nothing is hashed without one")
    dev = torch.device("cuda:0")
    res = {}
    for T, N, H, reverse in LSTM_CASES:
        x, w_ih, w_hh, bias = (None if t is None else t.to(dev) for t in lr.make_case("typical", T, N, H, seed=1))
        dh = tr.make_dh(T, N, H, seed=1).to(dev)
        h, saved = rnn.lstm_forward(x, w_ih, w_hh, bias, reverse)
        row = {"h": sha(h)}
        for need_bias in (True, False):
            out = rnn.lstm_backward(x, w_ih, w_hh, h, saved, dh, reverse, need_bias=need_bias)
            assert (out[3] is None) == (not need_bias)
            row.update({name + ("" if need_bias else "/no_db"): sha(t) for name, t in zip(("dx", "dw_ih", "dw_hh", "db"), out) if t is not None})
        res["lstm T=%d N=%d H=%d %s" % (T, N, H, "rev" if reverse else "fwd")] = row
    for i in CONV_ROWS:
        case = tl.CONV_CASES[i]
        x, w, b, dy, pad = tl.conv_inputs(case)
        x = x[:, :, 0].contiguous() if case[1] == 1 else x
        x, w, b, dy = x.to(dev), w.to(dev), b.to(dev), dy.to(dev)
        for clamp in (None, tl.CLAMP):
            y = train_ops.conv1d_forward(x, w, b, case[4], pad, "swish", clamp)
            dx, dw, db = train_ops.conv1d_backward(x, w, b, y, dy, case[4], pad, "swish", clamp)
            res["conv row %d %s" % (i, "clamped" if clamp else "free")] = {"y": sha(y), "dx": sha(dx), "dw": sha(dw), "db": sha(db)}
    for i in LINEAR_ROWS:
        case = tl.LINEAR_CASES[i]
        act, scale, clamp = case[4:7]
        x, w, b, dy = (None if t is None else t.to(dev) for t in tl.linear_inputs(case))
        for batch_major in (False, True):
            y = train_ops.linear_forward(x, w, b, act, scale, clamp, batch_major)
            dyd = dy.permute(1, 0, 2).contiguous() if batch_major else dy
            dx, dw, db = train_ops.linear_backward(x, w, y, dyd, act, scale, clamp, batch_major)
            res["linear row %d %s" % (i, "ntc" if batch_major else "tnc")] = {"y": sha(y), "dx": sha(dx), "dw": sha(dw), "db": sha(db)}
    if hasattr(train_ops, "rmsnorm_residual_backward"):        # a checkout from before the transformer family's layers has neither
        import transformer_train_ref as tt
        for M, D in NORM_CASES:
            c = {k: v.to(dev) for k, v in tt.norm_case(M, D).items()}
            out = train_ops.rmsnorm_residual_forward(c["a"], c["x"], c["w"], NORM_ALPHA)
            da, dx, dw = train_ops.rmsnorm_residual_backward(c["a"], c["x"], c["w"], c["dy"], NORM_ALPHA)
            res["norm M=%d D=%d" % (M, D)] = {"out": sha(out), "da": sha(da), "dx": sha(dx), "dw": sha(dw)}
        for M, D, F in GATED_CASES:
            c = {k: v.to(dev) for k, v in tt.gated_case(M, D, F).items()}
            h = train_ops.gated_linear_forward(c["x"], c["w"])
            dx, dw = train_ops.gated_linear_backward(c["x"], c["w"], c["dh"])
            res["gated M=%d D=%d F=%d" % (M, D, F)] = {"h": sha(h), "dx": sha(dx), "dw": sha(dw)}
    if hasattr(train_ops, "batchnorm_backward"):               # new keys: a checkout from before the layer has none of them
        import batchnorm_train_ref as bn
        for N, L, C, pad in BATCHNORM_CASES:
            c = {k: v.to(dev) for k, v in bn.bn_case(N, L, C - pad).items()}
            z, dy, gamma, beta = (torch.nn.functional.pad(c[k], (0, pad)) for k in ("z", "dy", "gamma", "beta"))
            for clamp, time_major in ((None, False), (bn.CLAMP, True)):
                rm, rv = c["running_mean"].clone(), c["running_var"].clone()
                y, mean, rstd = train_ops.batchnorm_forward(z, gamma, beta, rm, rv, bn.MOMENTUM, bn.EPS, "swish", clamp, time_major, C - pad)
                dyd = dy.permute(1, 0, 2).contiguous() if time_major else dy
                dz, dgamma, dbeta = train_ops.batchnorm_backward(z, gamma, beta, mean, rstd, y, dyd, "swish", clamp, time_major, C - pad)
                res["batchnorm N=%d L=%d C=%d-%d %s" % (N, L, C, pad, "clamped tm" if clamp else "free")] = {
                    "y": sha(y), "mean": sha(mean), "rstd": sha(rstd), "running_mean": sha(rm), "running_var": sha(rv), "dz": sha(dz),
                    "dgamma": sha(dgamma), "dbeta": sha(dbeta)}
    from bonito_amd.ctc import Model as CtcModel
    if hasattr(CtcModel, "forward_train"):                     # new keys: a checkout from before the QuartzNet forward_train has none of them
        for name, model, x, kwargs in model_cases():
            model = model.to(dev).train()
            scores = model.forward_train(x.to(dev), **kwargs)
            scores.backward(torch.randn(scores.shape, generator=torch.Generator().manual_seed(11)).half().to(dev))
            row = {"scores": sha(scores)}
            row.update({"grad " + k: sha(p.grad) for k, p in model.named_parameters()})
            row.update({k: sha(b) for k, b in model.named_buffers() if k.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked")})
            res[name] = row
    torch.cuda.synchronize()
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()

"""References of what training a QuartzNet CTC model adds (bh_dwconv1d_train_backward, bh_residual_act_train_*, bh_ctc_head_train_backward,
bonito_amd.train_ops.depthwise_conv1d / residual_act / ctc_head, bonito_amd.ctc.Model.forward_train): the references of
tests/test_gpu_quartznet_train.py and tests/test_gpu_quartznet_train_model.py, pinned by tests/test_quartznet_train_ref_cpu.py. Plain torch
and Python integers on the CPU; no import of bonito_amd.

    depthwise   y[n][t][c] = sum_k w[c][k] x[n][t + k - pad][c]                 x [N][L][C] channel-minor, w [C][1][K], stride 1
    residual    y = act(a + b) keep / (1 - p)                                   keep: the counter-based function below, never stored
    head        lp = log_softmax(x w^T + bias)                                  x [M][F], w [classes][F]

    formulas    the written-out forward and backward, in fp64
    exact       fp64 torch under autograd: F.conv1d(groups=C), log_softmax(conv1d(K = 1)), act(a + b) mask / (1 - p)
    yardstick   the same in fp16 on the CPU: how far half-precision training is from `exact`. The residual layer runs in torch.float16 as
                it is. The convolutions run as torch's fp16 kernels compute them - fp16 operands (the weights rounded to fp16, as
                autocast does), fp32 accumulation, every result and every gradient rounded to fp16 (round16 below) - because torch's CPU
                grouped convolution has no usable fp16 backward
    emulate     an fp32 statement of the device's design: fp32 products added unit by unit and block by block, the softmax recomputed in
                fp32, fp16 stores; with `defect` one planted mistake

dist(a, exact) = max|a - exact| / max|exact| in fp64. Every output must satisfy dist(kernel) <= 2 dist(yardstick).

The keep function, in 64-bit unsigned arithmetic (mod 2^64), as include/bonito_hip.h states it:
    mix(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
    keep(i) = (mix(mix(seed + G (stream_id + 1)) + G (i + 1)) >> 32) >= floor(p 2^32)         G = 0x9E3779B97F4A7C15
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from train_layers_ref import act_fn, act_grad, dist  # noqa: F401  (one definition of each)

F64 = torch.float64
MARGIN = 2.0
ACTS = ("none", "swish", "tanh", "relu")
DW_DEFECTS = ("taps_not_flipped", "pad_for_K_1_pad", "halo_dropped", "dw_first_item_only")
HEAD_DEFECTS = ("softmax_term_missing", "sum_over_8_lanes")
RES_DEFECTS = ("inv_keep_missing_backward", "other_stream_mask", "act_grad_at_a")

# the split of csrc/quartznet_train.hip: units of 64 rows of one chunk, tiles of 64 channels, about 1024 workgroups, 8 runs of blocks
UNIT, CTILE, WORKGROUPS, RUNS = 64, 64, 1024, 8
HEAD_MIN_ROWS, HEAD_MAX_BLOCKS = 64, 1024

# ---- the keep function ----------------------------------------------------------------------------------------------------------------------
MASK64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix(z):
    z &= MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


def p_threshold(p):
    """floor(p 2^32), computed in double; 0 <= p < 1."""
    if not 0.0 <= p < 1.0:
        raise ValueError("p must be in 0 <= p < 1")
    return int(math.floor(float(p) * 4294967296.0))


def keep_bits(seed, stream_id, index):
    """The top 32 bits an element is judged by, in Python integers."""
    key = mix(seed + GOLDEN * (stream_id + 1))
    return mix(key + GOLDEN * (index + 1)) >> 32


def keep(seed, stream_id, index, p):
    return keep_bits(seed, stream_id, index) >= p_threshold(p)


def keep_mask(seed, stream_id, n, p, start=0):
    """keep() of the indices start .. start + n - 1 -> bool tensor [n]; numpy uint64 (wrapping), pinned to keep() by the CPU tests."""
    key = np.uint64(mix(seed + GOLDEN * (stream_id + 1)))
    with np.errstate(over="ignore"):
        z = key + np.uint64(GOLDEN) * (np.arange(start, start + n, dtype=np.uint64) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return torch.from_numpy((z >> np.uint64(32)) >= np.uint64(p_threshold(p)))


# ---- depthwise convolution -----------------------------------------------------------------------------------------------------------------
def out_len(L, K, pad):
    return L + 2 * pad - K + 1


def dw_case(N, L, C, K, pad, seed=0):
    """-> {x fp16 [N][L][C], w fp32 [C][1][K], dy fp16 [N][Lout][C], pad}. Seeded."""
    g = torch.Generator().manual_seed(9900 + seed + 31 * C + 7 * L + 3 * K + N)
    return {"x": torch.randn(N, L, C, generator=g).half(), "w": torch.randn(C, 1, K, generator=g) / math.sqrt(K),
            "dy": (0.25 + torch.randn(N, out_len(L, K, pad), C, generator=g)).half(), "pad": pad}


def _shifted(t, lo, n):
    """rows lo .. lo + n - 1 of t [N][rows][C] along dim 1, zeros outside."""
    N, rows, C = t.shape
    out = torch.zeros(N, n, C, dtype=t.dtype)
    a, b = max(lo, 0), min(lo + n, rows)
    if b > a:
        out[:, a - lo:b - lo] = t[:, a:b]
    return out


def dw_formulas(case, dtype=F64):
    """The layer written out -> {y, dx, dw}."""
    x, w, dy, pad = case["x"].to(dtype), case["w"].to(dtype)[:, 0], case["dy"].to(dtype), case["pad"]
    N, L, C = x.shape
    K = w.shape[1]
    Lout = out_len(L, K, pad)
    y, dx, dw = torch.zeros(N, Lout, C, dtype=dtype), torch.zeros(N, L, C, dtype=dtype), torch.zeros(C, K, dtype=dtype)
    for k in range(K):
        xs = _shifted(x, k - pad, Lout)                       # x[n][t + k - pad][c]
        y += w[:, k] * xs
        dx += w[:, k] * _shifted(dy, pad - k, L)              # dy[n][p + pad - k][c]
        dw[:, k] = (dy * xs).sum((0, 1))
    return {"y": y, "dx": dx, "dw": dw[:, None, :]}


class _Round16(torch.autograd.Function):
    """A value as fp16 stores it, and its gradient as fp16 stores it."""

    @staticmethod
    def forward(ctx, t):
        return t.half().to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.half().to(g.dtype)


def round16(t):
    return _Round16.apply(t)


def _dw_autograd(case, dtype, rnd=lambda t: t):
    x = case["x"].to(dtype).permute(0, 2, 1).contiguous().requires_grad_()
    w = case["w"].to(dtype).clone().requires_grad_()
    y = rnd(F.conv1d(rnd(x), rnd(w), padding=case["pad"], groups=w.shape[0]))
    y.backward(case["dy"].to(dtype).permute(0, 2, 1))
    return {"y": y.detach().permute(0, 2, 1), "dx": x.grad.permute(0, 2, 1), "dw": w.grad}


def dw_exact(case):
    return _dw_autograd(case, F64)


def dw_yardstick(case):
    return {k: v.half() for k, v in _dw_autograd(case, torch.float32, round16).items()}


def dw_blocks(N, L, C, K, pad):
    """-> (units per chunk, units per block, blocks): the row split of the dw kernel, a function of the shape alone."""
    tiles = -(-out_len(L, K, pad) // UNIT)
    units = N * tiles
    b = min(max(WORKGROUPS // -(-C // CTILE), 1), units)
    per = -(-units // b)
    return tiles, per, -(-units // per)


def block_order_sum(parts):
    """fp32 [blocks][...] -> the blocks added in RUNS runs of consecutive blocks, each in block order, then the runs in order."""
    B = parts.shape[0]
    per = -(-B // RUNS)
    total = None
    for r in range(RUNS):
        run = torch.zeros_like(parts[0])
        for b in range(r * per, min((r + 1) * per, B)):
            run = run + parts[b]
        total = run if total is None else total + run
    return total


def dw_emulate(case, defect=None):
    """fp32 as the device computes: y and dx by multiply-adds in tap order with one rounding at the store, dw as fp32 sums of units of
    64 rows, the units of a block added in order and the blocks in block order."""
    f32 = torch.float32
    x, w, dy, pad = case["x"].to(f32), case["w"].to(f32)[:, 0], case["dy"].to(f32), case["pad"]
    N, L, C = x.shape
    K = w.shape[1]
    Lout = out_len(L, K, pad)
    y, dx = torch.zeros(N, Lout, C, dtype=f32), torch.zeros(N, L, C, dtype=f32)
    for k in range(K):
        y = y + w[:, k] * _shifted(x, k - pad, Lout)
        if defect == "taps_not_flipped":
            src = _shifted(dy, pad - (K - 1 - k), L)
        elif defect == "pad_for_K_1_pad":                       # the flipped convolution with padding pad instead of K - 1 - pad
            src = _shifted(dy, (K - 1 - pad) - k, L)
        else:
            src = _shifted(dy, pad - k, L)
        if defect == "halo_dropped":                            # a tile of 64 positions sees only its own 64 dy rows
            p = torch.arange(L)
            same = ((p + pad - k) // UNIT == p // UNIT) | (p + pad - k < 0)
            src = src * same[None, :, None]
        dx = dx + w[:, k] * src
    tiles, per, blocks = dw_blocks(N, L, C, K, pad)
    parts = torch.zeros(blocks, C, K, dtype=f32)
    for u in range(N * tiles):
        n, t0 = divmod(u, tiles)
        t0 *= UNIT
        rows = min(UNIT, Lout - t0)
        if defect == "dw_first_item_only" and n > 0:
            continue
        d = dy[n:n + 1, t0:t0 + rows]
        for k in range(K):
            xs = _shifted(x[n:n + 1], t0 + k - pad, rows)
            if defect == "halo_dropped":
                q = t0 + k - pad + torch.arange(rows)
                xs = xs * ((q >= t0) & (q < t0 + UNIT))[None, :, None]
            parts[u // per, :, k] += (d * xs).sum((0, 1))
    return {"y": y.half(), "dx": dx.half(), "dw": block_order_sum(parts)[:, None, :]}


# ---- residual add + activation + dropout ---------------------------------------------------------------------------------------------------------
def res_case(M, C, with_b=True, seed=0):
    g = torch.Generator().manual_seed(9950 + seed + 31 * C + M)
    return {"a": torch.randn(M, C, generator=g).half(), "b": torch.randn(M, C, generator=g).half() if with_b else None,
            "dy": (0.25 + torch.randn(M, C, generator=g)).half()}


def res_mask(case, p, seed, stream_id):
    M, C = case["a"].shape
    return keep_mask(seed, stream_id, M * C, p).reshape(M, C)


def res_formulas(case, act, p, mask, dtype=F64):
    a, dy = case["a"].to(dtype), case["dy"].to(dtype)
    u = a if case["b"] is None else a + case["b"].to(dtype)
    scale = mask.to(dtype) / (1.0 - p)
    return {"y": act_fn(u, act) * scale, "da": dy * scale * act_grad(u, act)}


def _res_autograd(case, act, p, mask, dtype):
    a = case["a"].to(dtype).clone().requires_grad_()
    b = None if case["b"] is None else case["b"].to(dtype).clone().requires_grad_()
    y = act_fn(a if b is None else a + b, act) * mask.to(dtype) / (1.0 - p)
    y.backward(case["dy"].to(dtype))
    if b is not None:
        assert torch.equal(a.grad, b.grad)
    return {"y": y.detach(), "da": a.grad}


def res_exact(case, act, p, mask):
    return _res_autograd(case, act, p, mask, F64)


def res_yardstick(case, act, p, mask):
    return _res_autograd(case, act, p, mask, torch.float16)


def res_emulate(case, act, p, seed, stream_id, defect=None):
    f32 = torch.float32
    a, dy = case["a"].to(f32), case["dy"].to(f32)
    u = a if case["b"] is None else a + case["b"].to(f32)
    keep_f = res_mask(case, p, seed, stream_id).to(f32)
    inv = torch.tensor(1.0 / (1.0 - p), dtype=f32)
    y = act_fn(u, act) * inv * keep_f
    keep_b = res_mask(case, p, seed, stream_id + 1).to(f32) if defect == "other_stream_mask" else keep_f
    at = a if defect == "act_grad_at_a" else u
    da = dy * (1.0 if defect == "inv_keep_missing_backward" else inv) * act_grad(at, act) * keep_b
    return {"y": y.half(), "da": da.half()}


# ---- CTC head -----------------------------------------------------------------------------------------------------------------------------------
def head_case(M, Fe, classes, seed=0):
    """-> {x fp16 [M][F], w fp32 [classes][F], b fp32 [classes], dlp fp16 [M][classes]}. Seeded; dlp with a mean, so that its row sums and
    with them the softmax term do not vanish."""
    g = torch.Generator().manual_seed(9970 + seed + 31 * Fe + 7 * classes + M)
    return {"x": torch.randn(M, Fe, generator=g).half(), "w": torch.randn(classes, Fe, generator=g) / math.sqrt(Fe),
            "b": 0.3 * torch.randn(classes, generator=g), "dlp": (0.5 + torch.randn(M, classes, generator=g)).half()}


def head_formulas(case, dtype=F64):
    x, w, b, dlp = (case[k].to(dtype) for k in ("x", "w", "b", "dlp"))
    logit = x @ w.T + b
    lp = logit - torch.logsumexp(logit, 1, keepdim=True)
    dlogit = dlp - lp.exp() * dlp.sum(1, keepdim=True)
    return {"lp": lp, "dx": dlogit @ w, "dw": dlogit.T @ x, "db": dlogit.sum(0)}


def _head_autograd(case, dtype, rnd=lambda t: t):
    x = case["x"].to(dtype).T[None].contiguous().requires_grad_()                  # [1][F][M]
    w = case["w"].to(dtype)[:, :, None].clone().requires_grad_()
    b = case["b"].to(dtype).clone().requires_grad_()
    lp = rnd(torch.log_softmax(rnd(F.conv1d(rnd(x), rnd(w), rnd(b))), dim=1))      # [1][classes][M]
    lp.backward(case["dlp"].to(dtype).T[None])
    return {"lp": lp.detach()[0].T, "dx": x.grad[0].T, "dw": w.grad[:, :, 0], "db": b.grad}


def head_exact(case):
    return _head_autograd(case, F64)


def head_yardstick(case):
    return {k: v.half() for k, v in _head_autograd(case, torch.float32, round16).items()}


def head_block_rows(M):
    return max(HEAD_MIN_ROWS, -(-M // HEAD_MAX_BLOCKS))


def head_emulate(case, defect=None):
    """fp32: the softmax recomputed from x, w, bias (never from the stored fp16 lp), dx rounded once, dw and db as sums of row blocks
    added in block order."""
    f32 = torch.float32
    x, w, b, dlp = (case[k].to(f32) for k in ("x", "w", "b", "dlp"))
    M, classes = dlp.shape
    logit = x @ w.T + b
    lp = logit - torch.logsumexp(logit, 1, keepdim=True)
    g = dlp.sum(1, keepdim=True)
    if defect == "sum_over_8_lanes":                                               # 8 lanes read from the row's start: the next row's values ride along
        flat = torch.cat([dlp.reshape(-1), torch.zeros(8, dtype=f32)])
        g = torch.stack([flat[m * classes:m * classes + 8].sum() for m in range(M)])[:, None]
    dlogit = dlp if defect == "softmax_term_missing" else dlp - lp.exp() * g
    rows = head_block_rows(M)
    blocks = -(-M // rows)
    pw, pb = torch.zeros(blocks, classes, x.shape[1], dtype=f32), torch.zeros(blocks, classes, dtype=f32)
    for i in range(blocks):
        d, xb = dlogit[i * rows:(i + 1) * rows], x[i * rows:(i + 1) * rows]
        pw[i], pb[i] = d.T @ xb, d.sum(0)
    return {"lp": lp.half(), "dx": (dlogit @ w).half(), "dw": block_order_sum(pw), "db": block_order_sum(pb)}


def within(got, exact, yard, names, label="", margin=MARGIN, say=print):
    """Every named output within margin x the yardstick's distance; prints each figure first. -> the list of names that are not."""
    bad = []
    for name in names:
        dk, dy = dist(got[name], exact[name]), dist(yard[name], exact[name])
        say("%s %-4s: dist = %.3e  dist(yardstick) = %.3e  ratio = %.3f" % (label, name, dk, dy, dk / dy if dy > 0 else (0.0 if dk == 0 else float("inf"))))
        if not dk <= margin * dy:
            bad.append(name)
    return bad

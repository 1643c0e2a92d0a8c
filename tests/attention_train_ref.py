"""References of the training attention layer (bh_attention_train_forward / bh_attention_train_backward, bonito_amd.attn): the references of
tests/test_gpu_attention_train.py and tests/test_gpu_attention_module.py, pinned by tests/test_attention_train_ref_cpu.py. Host only; builds
on tests/attention_ref.py (mask, rotary, rounding); no import of bonito_amd.

Per (chunk, head), with q~ = rot(q) / 8, k~ = rot(k), s_ij = q~_i . k~_j on the visible pairs (i - wl <= j <= i + wr),
lse_i = ln sum_j exp(s_ij), P_ij = exp(s_ij - lse_i), O = P V and delta_i = sum_d dO_id O_id:

    dV_j = sum_i P_ij dO_i        dP_ij = dO_i . V_j        dS_ij = P_ij (dP_ij - delta_i)
    dq~_i = sum_j dS_ij k~_j      dk~_j = sum_i dS_ij q~_i  dq = rot^-1(dq~) / 8        dk = rot^-1(dk~)

    exact(qkv, dout, window)                      -> (out, dq, dk, dv) float64 from these formulas, no autograd in them
    exact(..., storage_fp16=True)                 the same with a rounding to fp16 exactly where bonito_amd/csrc/attention_train.hip rounds:
                                                  q~ and k~ (MFMA operands), the normalised probabilities of the forward's PV product and the
                                                  forward's output (attention_ref's general kernel), P as the operand of dV, dS as the operand
                                                  of dq~ and dk~, and dq, dk, dv once at the store; delta from the rounded O. Everything else fp64.
    exact(..., storage_fp16=True, fp32_places=True)
                                                  additionally the two places where the kernels' fp32 arithmetic is not small beside their fp16
                                                  storage. Both show where a query puts all its weight on one key: P = 1 and dP - delta = 0 (a single
                                                  visible key) or nearly so (the probes of tests/attention_train_cases.py that must not be seen)
                                                  whatever q~ and k~ round to, so the fp16 roundings above cost nothing, d16 would be 0 and 4 d16
                                                  unattainable for a correct kernel.
                                                  (1) dS = P (dP - delta) is the difference of two fp32 sums of 64 products taken in different
                                                  orders, dP by the MFMA chain and delta sequentially (attn_delta_kernel): here dP is the fp64 sum
                                                  rounded once to fp32 and delta the kernel's own sequential fp32 sum (feature 0 first; a product
                                                  of two fp16 values is exact in fp32).
                                                  (2) q~ and k~ are rounded to fp16 TWICE, by the forward (which leaves lse and out) and again by
                                                  the backward passes (which recompute s), from fp32 rotations a co - b si that the compiler fuses
                                                  into one multiply-add at some sites and elements and not at others (csrc/attn_block.h says so,
                                                  and the forward's bytes are pinned): the two fp32 values differ in their last bit, and about one
                                                  element in 2^13 rounds to the other fp16 neighbour. exp(s - lse) is then the forward's
                                                  probability times exp(ulp16(q~) k~): 1 - 2^-11 instead of 1 once |q~| reaches 4. Here the
                                                  forward's q~, k~ come from the unfused fp32 rotation and the backward's from the fused one
                                                  (cos and sin rounded to fp32, as in the kernels' table).
                                                  The probe sweep measures its d16 with this; the Gaussian cases keep the plain form.
    exact(..., stats=True)                        appends lse and delta [N, H, T] (the layout of the kernels' planes) to the result
    exact(..., defect=NAME)                       a planted defect (DEFECTS, WINDOW_DEFECTS), for the test that the bound would catch it.
                                                  WINDOW_DEFECTS are wrong decisions about single (query, key) pairs: drop_left (both passes lose
                                                  the key at -wl), unmirrored (the key pass walks j - wl .. j + wr), drop_right_key_pass (the key
                                                  pass loses the query at j - wr), seam_leak (the query pass ignores the chunk bounds and meets the
                                                  rows of the chunks stored in front of and behind its own)
    autograd(qkv, dout, window)                   fp64 torch autograd through rotary + masked softmax attention
    dist(a, e) = max|a - e| / max|e|;  d16 of a case = dist(exact(storage_fp16=True), exact()) per part: what fp16 storage costs a
    correct kernel. The device test requires dist(kernel, exact) <= 4 d16 per part (the project's rule for attention,
    tests/test_gpu_attention.py: fp32 accumulation in another order, hardware exp).

    mha_exact / mha_yardstick                     the reference's MultiHeadAttention.forward (Wqkv, rotary, scaled_dot_product_attention under the
                                                  band mask, out_proj) restated in torch, with autograd: in fp64, and in fp16 on the CPU.
"""
import numpy as np
import torch

import attention_ref as ar

HEAD_DIM = ar.HEAD_DIM
PARTS = ("dq", "dk", "dv")
DEFECTS = ("no_delta", "no_scale", "rot_forward", "unmirrored", "drop_left")
WINDOW_DEFECTS = ("drop_left", "unmirrored", "drop_right_key_pass", "seam_leak")          # wrong decisions about one (query, key) pair


def make_case(N, T, H, kind="gauss", seed=0):
    """-> (qkv fp16 [N, T, 3, H, 64], dout fp16 [N, T, H*64]) as numpy: Gaussian (sigma 0.7), `peaked` with q times 3; dout ~ N(0, 1)."""
    rng = np.random.default_rng(9100 + seed)
    qkv = rng.normal(0.0, 0.7, (N, T, 3, H, HEAD_DIM))
    if kind == "peaked":
        qkv[:, :, 0] *= 3.0
    else:
        assert kind == "gauss"
    dout = rng.normal(0.0, 1.0, (N, T, H * HEAD_DIM))
    return qkv.astype(np.float16), dout.astype(np.float16)


def _rot(x, inverse=False):
    """x [T, 64] -> rotated along T."""
    return ar.rotate(x[None, :, None, :], inverse)[0, :, 0]


def _delta32(do, out):
    """attn_delta_kernel's sum: fp32, sequential over the 64 features; do, out [T, 64] hold fp16 values, so every product is exact in fp32."""
    acc = np.zeros(do.shape[0], np.float32)
    for d in range(do.shape[1]):
        acc = acc + (do[:, d] * out[:, d]).astype(np.float32)
    assert acc.dtype == np.float32
    return acc.astype(np.float64)[:, None]


def _rot32(x, fused):
    """x [T, 64] fp16 values -> the rotation as the kernels form it in fp32 from the fp32 table: a co - b si and a si + b co with the first
    product fused into the subtraction / addition (one rounding) or not (two). float64 holding fp32 values."""
    ang = ar.rotary_angles(x.shape[0], x.shape[1])
    co, si = np.cos(ang).astype(np.float32).astype(np.float64), np.sin(ang).astype(np.float32).astype(np.float64)
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    a, b = x[:, :x.shape[1] // 2], x[:, x.shape[1] // 2:]
    first = (lambda p: p) if fused else f32                   # a fp16 value times a fp32 value is exact in fp64
    return np.concatenate([f32(first(a * co) - f32(b * si)), f32(first(a * si) + f32(b * co))], axis=1)


def _one(q, k, v, do, window, s16, defect, fp32_places=False, stats=False):
    """One (chunk, head): q, k, v, do [T, 64] float64 -> (out, dq, dk, dv) [T, 64]; stats: also (lse, delta) [T]."""
    T = q.shape[0]
    wl, wr = window
    rnd = ar.r16 if s16 else (lambda a: a)
    mask = ar.visible(T, window)
    qt, kt = rnd(_rot(q) * 0.125), rnd(_rot(k))
    if fp32_places:
        assert s16, "the fp32 places belong to the fp16-storage form"
        qt, kt = rnd(_rot32(q, False) * 0.125), rnd(_rot32(k, False))          # the forward's
    out = ar.attend_one(qt, kt, v, mask, False, "normalised" if s16 else None, s16)
    s = np.where(mask, qt @ kt.T, -np.inf)
    m = s.max(axis=1, keepdims=True)
    lse = m + np.log(np.exp(s - m).sum(axis=1, keepdims=True))
    if fp32_places:
        qt, kt = rnd(_rot32(q, True) * 0.125), rnd(_rot32(k, True))            # the backward's
    delta = (do * out).sum(axis=1, keepdims=True)
    dp = do @ v.T
    if fp32_places:
        delta, dp = _delta32(do, out), dp.astype(np.float32).astype(np.float64)
    if defect == "no_delta":
        delta = np.zeros_like(delta)

    def p_ds(msk):
        p = np.where(msk, np.exp(np.where(msk, qt @ kt.T, 0.0) - lse), 0.0)
        return p, p * (dp - delta)

    mq = mk = mask
    i, j = np.arange(T)[:, None], np.arange(T)[None, :]
    if defect == "drop_left":                     # the key at offset -wl is lost by both passes
        mq = mk = mask & (j != i - wl)
    if defect == "unmirrored":                    # the key pass walks the queries j - wl .. j + wr instead of j - wr .. j + wl
        mk = ar.visible(T, (wr, wl))
    if defect == "drop_right_key_pass":           # the key pass loses the query at j - wr
        mk = mask & (i != j - wr)
    _, ds_q = p_ds(mq)
    p_k, ds_k = p_ds(mk)
    dqt = rnd(ds_q) @ kt
    dkt = rnd(ds_k).T @ qt
    dv = rnd(p_k).T @ do
    back = defect != "rot_forward"
    dq = _rot(dqt, inverse=back) * (1.0 if defect == "no_scale" else 0.125)
    dk = _rot(dkt, inverse=back)
    res = (out, rnd(dq), rnd(dk), rnd(dv))
    return res + (lse[:, 0], delta[:, 0]) if stats else res


def _leaky_query_pass(q, k, v, do, lse, delta, window, s16):
    """The planted defect `seam_leak`: the query pass of one head with the chunk bounds ignored. The rows of all chunks are contiguous in
    memory, so query i of chunk n then also meets the rows of chunk n - 1 and n + 1 that lie at the memory positions i - wl .. i + wr (each
    rotated by its own position in its own chunk, as it is stored). lse and delta are the correct forward's. q, k, v, do [N, T, 64],
    lse, delta [N, T] -> dq [N, T, 64]."""
    N, T, d = q.shape
    rnd = ar.r16 if s16 else (lambda a: a)
    qt = np.stack([rnd(_rot(q[n]) * 0.125) for n in range(N)]).reshape(N * T, d)
    kt = np.stack([rnd(_rot(k[n])) for n in range(N)]).reshape(N * T, d)
    band = ar.visible(N * T, window)
    p = np.where(band, np.exp(np.where(band, qt @ kt.T, 0.0) - lse.reshape(-1, 1)), 0.0)
    ds = p * (do.reshape(N * T, d) @ v.reshape(N * T, d).T - delta.reshape(-1, 1))
    dqt = (rnd(ds) @ kt).reshape(N, T, d)
    return np.stack([rnd(_rot(dqt[n], inverse=True) * 0.125) for n in range(N)])


def exact(qkv, dout, window, storage_fp16=False, defect=None, fp32_places=False, stats=False):
    """qkv [N, T, 3, H, 64], dout [N, T, H*64] (the fp16 values the kernels are given) -> (out [N, T, H*64], dq, dk, dv [N, T, H, 64]) float64;
    stats: also (lse, delta) [N, H, T]."""
    assert defect is None or defect in DEFECTS + WINDOW_DEFECTS
    qkv = np.asarray(qkv, np.float64)
    N, T, three, H, d = qkv.shape
    assert three == 3 and d == HEAD_DIM
    do = np.asarray(dout, np.float64).reshape(N, T, H, d)
    res = [np.zeros((N, T, H, d)) for _ in range(4)]
    planes = [np.zeros((N, H, T)) for _ in range(2)]
    for n in range(N):
        for h in range(H):
            parts = _one(qkv[n, :, 0, h], qkv[n, :, 1, h], qkv[n, :, 2, h], do[n, :, h], window, storage_fp16,
                         None if defect == "seam_leak" else defect, fp32_places, True)
            for r, p in zip(res, parts):
                r[n, :, h] = p
            for r, p in zip(planes, parts[4:]):
                r[n, h] = p
    if defect == "seam_leak":
        for h in range(H):
            res[1][:, :, h] = _leaky_query_pass(qkv[:, :, 0, h], qkv[:, :, 1, h], qkv[:, :, 2, h], do[:, :, h], planes[0][:, h], planes[1][:, h],
                                                window, storage_fp16)
    return (res[0].reshape(N, T, H * d),) + tuple(res[1:]) + (tuple(planes) if stats else ())


def dist(a, e):
    """max|a - e| / max|e| in fp64 (0 / 0 = 0; a non-finite a is inf)."""
    a, e = np.asarray(a, np.float64), np.asarray(e, np.float64)
    if not np.isfinite(a).all():
        return float("inf")
    err, ref = float(np.abs(a - e).max()), float(np.abs(e).max())
    return 0.0 if err == 0.0 else err / ref if ref > 0 else float("inf")


def d16(qkv, dout, window, want=None):
    """{part: dist(exact with fp16 storage, exact)} for dq, dk, dv."""
    want = exact(qkv, dout, window) if want is None else want
    got = exact(qkv, dout, window, storage_fp16=True)
    return {name: dist(g, w) for name, g, w in zip(PARTS, got[1:], want[1:])}


def split(dqkv):
    """packed gradient [N, T, 3, H, 64] (or [N, T, 3*H*64]) -> (dq, dk, dv) [N, T, H, 64] float64."""
    g = np.asarray(dqkv, np.float64)
    g = g.reshape(g.shape[0], g.shape[1], 3, -1, HEAD_DIM)
    return g[:, :, 0], g[:, :, 1], g[:, :, 2]


def single_key_bounds(qkv, dout):
    """A window under which every query sees exactly one key, itself ((0, 0), or T = 1): P = 1, out = v, dv = dout, and the exact dq and dk
    are 0 - d16 is 0, so the kernels are held to a derived bound instead. dS_i = dP_i - delta_i is the difference of two fp32 dot products of
    the same 64 terms dO_id V_id in different orders (an MFMA chain, a sequential sum): each within 64 2^-24 sum_d |dO_id V_id| of the true
    sum, so |dS_i| <= 2 64 2^-24 sum_d |dO_id V_id|. dS is rounded to fp16 (relative 2^-11, or half a subnormal step 2^-25), multiplied by
    k~ (dq~) or q~ (dk~) - one product per feature, no sum - rotated back (each output a combination of the feature and its partner with
    |cos|, |sin| <= 1), scaled (dq) and rounded to fp16 once more; the fp32 roundings in between are covered by a factor 1 + 2^-10.
    -> (bound on |dq|, bound on |dk|) [N, T, H, 64]."""
    qkv = np.asarray(qkv, np.float64)
    N, T, three, H, d = qkv.shape
    do = np.asarray(dout, np.float64).reshape(N, T, H, d)
    qt, kt = ar.r16(ar.rotate(qkv[:, :, 0]) * 0.125), ar.r16(ar.rotate(qkv[:, :, 1]))
    ds = 2 * 64 * 2.0 ** -24 * np.abs(do * qkv[:, :, 2]).sum(axis=-1, keepdims=True)
    ds = ds * (1 + 2.0 ** -11) + 2.0 ** -25

    def carried(x, scale):
        pair = np.concatenate([x[..., d // 2:], x[..., :d // 2]], axis=-1)
        return (ds * (np.abs(x) + np.abs(pair)) * scale * (1 + 2.0 ** -10)) * (1 + 2.0 ** -11) + 2.0 ** -25

    return carried(kt, 0.125), carried(qt, 1.0)


# ---- torch restatements ----------------------------------------------------------------------------------------------------------------

def _band(T, window):
    return torch.from_numpy(ar.visible(T, window))


def _torch_rotary(x, dtype):
    """x [N, T, H, 64] -> rotary embedding (non-interleaved), cos / sin of attention_ref.rotary_angles cast to `dtype`."""
    T, d = x.shape[1], x.shape[-1]
    ang = torch.from_numpy(ar.rotary_angles(T, d))
    cos, sin = torch.cos(ang).to(dtype)[None, :, None, :], torch.sin(ang).to(dtype)[None, :, None, :]
    x1, x2 = x[..., :d // 2], x[..., d // 2:]
    return torch.cat([x1 * cos - x2 * sin, x1 * sin + x2 * cos], dim=-1)


def _torch_attention(qkv, window, dtype):
    """qkv [N, T, 3, H, 64] torch -> [N, T, H*64]: rotary on q and k, then the reference's scaled_dot_product_attention branch."""
    N, T = qkv.shape[:2]
    q, k, v = _torch_rotary(qkv[:, :, 0], dtype), _torch_rotary(qkv[:, :, 1], dtype), qkv[:, :, 2]
    q, k, v = (t.permute(0, 2, 1, 3) for t in (q, k, v))                  # [N, H, T, 64]
    o = torch.nn.functional.scaled_dot_product_attention(q, k, v, attn_mask=_band(T, window))
    return o.permute(0, 2, 1, 3).reshape(N, T, -1)


def autograd(qkv, dout, window):
    """fp64 torch autograd through rotary + masked softmax attention -> (out, dq, dk, dv) numpy float64."""
    x = torch.from_numpy(np.asarray(qkv, np.float64)).clone().requires_grad_()
    out = _torch_attention(x, window, torch.float64)
    out.backward(torch.from_numpy(np.asarray(dout, np.float64)))
    g = x.grad.numpy()
    return out.detach().numpy(), g[:, :, 0], g[:, :, 1], g[:, :, 2]


MHA_NAMES = ("y", "dx", "dWqkv", "dbqkv", "dWo", "dbo")


def make_mha_case(N, T, D, qkv_bias=False, seed=0):
    """-> dict of torch tensors: x fp16 [N, T, D] ~ N(0, 1), Wqkv [3D, D] and Wo [D, D] fp32 (xavier-like, std 1 / sqrt(D)), biases fp32
    (std 0.1; bqkv None without qkv_bias), dy fp16 [N, T, D] ~ N(0, 1)."""
    g = torch.Generator().manual_seed(9300 + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    return {"x": r(N, T, D).half(), "wqkv": r(3 * D, D) / D ** 0.5, "bqkv": 0.1 * r(3 * D) if qkv_bias else None,
            "wo": r(D, D) / D ** 0.5, "bo": 0.1 * r(D), "dy": r(N, T, D).half()}


def _mha(case, nhead, window, dtype):
    leaves = {k: (None if v is None else v.to(dtype).clone().requires_grad_()) for k, v in case.items() if k != "dy"}
    x = leaves["x"]
    N, T, D = x.shape
    lin = torch.nn.functional.linear
    qkv = lin(x, leaves["wqkv"], leaves["bqkv"]).view(N, T, 3, nhead, D // nhead)
    y = lin(_torch_attention(qkv, window, dtype), leaves["wo"], leaves["bo"])
    y.backward(case["dy"].to(dtype))
    grad = lambda k: None if leaves[k] is None else leaves[k].grad.to(torch.float64)
    return y.detach().to(torch.float64), grad("x"), grad("wqkv"), grad("bqkv"), grad("wo"), grad("bo")


def mha_exact(case, nhead, window):
    """fp64 restatement of the reference's MultiHeadAttention.forward with autograd -> (y, dx, dWqkv, dbqkv or None, dWo, dbo) float64."""
    return _mha(case, nhead, window, torch.float64)


def mha_yardstick(case, nhead, window):
    """The same restatement run by torch in fp16 on the CPU with its autograd: the measure of how far half-precision training is from
    mha_exact on a given case. The device test requires dist(kernel) <= 2 dist(yardstick) per part."""
    return _mha(case, nhead, window, torch.float16)

"""References of what a transformer encoder layer adds to training (bh_rmsnorm_train_backward, bh_gated_linear_train_*,
bonito_amd.train_ops.rmsnorm_residual / gated_linear, bonito_amd.attn.encoder_layer) and of the transformer chain
SeqdistModel.forward_train builds: the references of tests/test_gpu_transformer_train.py and tests/test_gpu_transformer_train_model.py,
pinned by tests/test_transformer_train_ref_cpu.py. Host only; builds on tests/attention_train_ref.py (rotary + band-masked attention in
torch); no import of bonito_amd.

    norm     z = a + alpha x    r = rsqrt(mean_d z^2 + eps)    out = z r w
             g = dy w    c = (1/D) sum_d g_d z_d    dz = r g - r^3 c z    da = dz    dx = alpha dz    dw_d = sum_m dy z r
    gated    [y | gate] = x W^T (W [2F][D], y rows first)    h = y gate sigmoid(gate)
             s = sigmoid(gate)    dy = dh gate s    dgate = dh y s (1 + gate (1 - s))    du = [dy | dgate]    dx = du W    dW = du^T x

    *_formulas(...)                 these formulas written out in numpy, no autograd: in float64, or - `emulate` - the device's design in
                                    float32 with a rounding to fp16 wherever it stores fp16 (out, da, dx; the recomputed u, du, h, dx);
                                    `defect`: one planted mistake (NORM_DEFECTS, GATED_DEFECTS)
    *_torch(case, dtype)            the layer restated in torch ops with autograd: `exact` in float64, the yardstick in float16 on the CPU
    layer_torch / model_torch       the whole encoder layer / the whole transformer chain restated in torch, in float64 or float16

dist(a, exact) = max|a - exact| / max|exact| in fp64. The device tests require dist(kernel) <= 2 dist(yardstick) per output: the
project's margin for composed training layers (tests/train_layers_ref.py). Parameters of every case are fp16-representable, so that a
layer that rounds its weights and one that reads them as fp32 (the norm's gain) are measured against the same exact values.
"""
import numpy as np
import torch
import torch.nn.functional as F

import attention_train_ref as tr

F64 = torch.float64
MARGIN = 2.0
EPS = 1e-5
NORM_DEFECTS = ("r3_term_dropped", "alpha_missing_on_dx", "w_missing_from_g", "mean_over_the_vector_count")
GATED_DEFECTS = ("gate_term_dropped", "halves_swapped", "interleaved_rows")
NORM_NAMES = ("out", "da", "dx", "dw")
GATED_NAMES = ("h", "dx", "dw")


def dist(a, want):
    """max|a - want| / max|want| in fp64 (0 / 0 = 0; a non-finite a is inf); numpy arrays or torch tensors."""
    a, want = (t.detach().to(F64).cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, np.float64) for t in (a, want))
    return tr.dist(a, want)


def _r16(t):
    return t.half().float()


# ---- norm -----------------------------------------------------------------------------------------------------------------------------------
def norm_case(M, D, seed=0, zero_row=None):
    """-> {a, x, dy fp16 [M][D] ~ N(0, 1); w fp32 [D] ~ 1 + 0.3 N(0, 1), fp16-representable}; `zero_row`: that row of a and x is zero."""
    g = torch.Generator().manual_seed(9700 + seed + 31 * D + M)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    case = {"a": r(M, D).half(), "x": r(M, D).half(), "w": _r16(1.0 + 0.3 * r(D)), "dy": r(M, D).half()}
    if zero_row is not None:
        case["a"][zero_row] = 0
        case["x"][zero_row] = 0
    return case


def norm_formulas(case, alpha, eps=EPS, emulate=False, defect=None):
    """-> (out, da, dx, dw) numpy: float64, or with `emulate` float32 with out, da, dx rounded to fp16 at the store."""
    assert defect is None or defect in NORM_DEFECTS
    ft = np.float32 if emulate else np.float64
    a, x, w, dy = (case[k].numpy().astype(ft) for k in ("a", "x", "w", "dy"))
    D = a.shape[1]
    alpha, eps = ft(alpha), ft(eps)
    z = a + alpha * x
    r = ft(1) / np.sqrt((z * z).mean(axis=1, keepdims=True, dtype=ft) + eps)
    out = z * r * w
    g = dy if defect == "w_missing_from_g" else dy * w
    c = (g * z).sum(axis=1, keepdims=True, dtype=ft) / ft(D // 8 if defect == "mean_over_the_vector_count" else D)
    dz = r * g - (ft(0) if defect == "r3_term_dropped" else r * r * r * c * z)
    da, dx = dz, dz if defect == "alpha_missing_on_dx" else alpha * dz
    dw = (dy * z * r).sum(axis=0, dtype=ft)
    if emulate:
        out, da, dx = (t.astype(np.float16).astype(np.float32) for t in (out, da, dx))
    return out, da, dx, dw


def _rms(z, w, eps):
    return z * torch.rsqrt(z.pow(2).mean(-1, keepdim=True) + eps) * w


def norm_torch(case, alpha, eps=EPS, dtype=F64):
    """RMSNorm(a + alpha x) in torch ops with autograd, in `dtype` -> (out, da, dx, dw) float64 tensors."""
    a, x, w = (case[k].to(dtype).clone().requires_grad_() for k in ("a", "x", "w"))
    out = _rms(a + alpha * x, w, eps)
    out.backward(case["dy"].to(dtype))
    return tuple(t.detach().to(F64) for t in (out, a.grad, x.grad, w.grad))


# ---- gated layer ----------------------------------------------------------------------------------------------------------------------------
def gated_case(M, D, F_, seed=0):
    """-> {x fp16 [M][D] ~ N(0, 1); w fp32 [2F][D] ~ N(0, 1) / sqrt(D), fp16-representable, the gate rows twice as large - y rows and gate
    rows get visibly different gradients; dh fp16 [M][F] ~ N(0, 1)}."""
    g = torch.Generator().manual_seed(9800 + seed + 31 * D + 7 * F_ + M)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    w = r(2 * F_, D) / D ** 0.5
    w[F_:] *= 2.0
    return {"x": r(M, D).half(), "w": _r16(w), "dh": r(M, F_).half()}


def gated_formulas(case, emulate=False, defect=None):
    """-> (h, dx, dw) numpy: float64, or with `emulate` float32 with h, the recomputed u, du and dx rounded to fp16 where the device stores
    them (h from the unrounded accumulators, as the GEMM's epilogue has them)."""
    assert defect is None or defect in GATED_DEFECTS
    ft = np.float32 if emulate else np.float64
    rnd = (lambda t: t.astype(np.float16).astype(np.float32)) if emulate else (lambda t: t)
    x, w, dh = (case[k].numpy().astype(ft) for k in ("x", "w", "dh"))
    Fh = w.shape[0] // 2
    sig = lambda t: ft(1) / (ft(1) + np.exp(-t))      # noqa: E731
    lo, hi = (slice(Fh, None), slice(None, Fh)) if defect == "halves_swapped" else (slice(None, Fh), slice(Fh, None))
    u = x @ w.T
    h = rnd(u[:, lo] * u[:, hi] * sig(u[:, hi]))
    u = rnd(u)
    y, gate = u[:, lo], u[:, hi]
    s = sig(gate)
    du = np.empty_like(u)
    du[:, lo] = dh * gate * s
    du[:, hi] = dh * y * s * (ft(1) if defect == "gate_term_dropped" else ft(1) + gate * (ft(1) - s))
    du = rnd(du)
    dx = rnd(du @ w)
    dw = du.T @ x
    if defect == "interleaved_rows":      # rows (dy_0, dgate_0, dy_1, ...): the layout of the forward's weights, not torch's
        dw = np.stack([dw[:Fh], dw[Fh:]], axis=1).reshape(2 * Fh, -1)
    return h, dx, dw


def gated_torch(case, dtype=F64):
    """fc1 + SwiGLU in torch ops with autograd, in `dtype` -> (h, dx, dw) float64 tensors."""
    x, w = (case[k].to(dtype).clone().requires_grad_() for k in ("x", "w"))
    y, gate = F.linear(x, w).chunk(2, dim=-1)
    h = y * F.silu(gate)
    h.backward(case["dh"].to(dtype))
    return tuple(t.detach().to(F64) for t in (h, x.grad, w.grad))


# ---- the whole encoder layer ------------------------------------------------------------------------------------------------------------------
LAYER_PARAMS = ("self_attn.Wqkv.weight", "self_attn.out_proj.weight", "self_attn.out_proj.bias", "norm1.weight", "ff.fc1.weight",
                "ff.fc2.weight", "norm2.weight")


def layer_case(N, T, D, F_, seed=0):
    """-> {x, dy fp16 [N][T][D]; the parameters of a TransformerEncoderLayer under their names, fp32 and fp16-representable}."""
    g = torch.Generator().manual_seed(9900 + seed + D + F_)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    p = {"self_attn.Wqkv.weight": r(3 * D, D) / D ** 0.5, "self_attn.out_proj.weight": r(D, D) / D ** 0.5, "self_attn.out_proj.bias": 0.1 * r(D),
         "norm1.weight": 1.0 + 0.3 * r(D), "ff.fc1.weight": r(2 * F_, D) / D ** 0.5, "ff.fc2.weight": r(D, F_) / F_ ** 0.5,
         "norm2.weight": 1.0 + 0.3 * r(D)}
    case = {k: _r16(v) for k, v in p.items()}
    case.update(x=r(N, T, D).half(), dy=r(N, T, D).half())
    return case


def layer_forward(p, x, nhead, window, alpha, eps, dtype, prefix=""):
    """The reference's TransformerEncoderLayer.forward on torch leaves p[prefix + name] in `dtype`, x [N][T][D]."""
    N, T, D = x.shape
    qkv = F.linear(x, p[prefix + "self_attn.Wqkv.weight"]).view(N, T, 3, nhead, D // nhead)
    a = F.linear(tr._torch_attention(qkv, window, dtype), p[prefix + "self_attn.out_proj.weight"], p[prefix + "self_attn.out_proj.bias"])
    x1 = _rms(a + alpha * x, p[prefix + "norm1.weight"], eps)
    y, gate = F.linear(x1, p[prefix + "ff.fc1.weight"]).chunk(2, dim=-1)
    f = F.linear(y * F.silu(gate), p[prefix + "ff.fc2.weight"])
    return _rms(f + alpha * x1, p[prefix + "norm2.weight"], eps)


def layer_torch(case, nhead, window, alpha, eps=EPS, dtype=F64):
    """-> {"y", "dx", and every name of LAYER_PARAMS: its gradient} float64 tensors."""
    leaves = {k: v.to(dtype).clone().requires_grad_() for k, v in case.items() if k != "dy"}
    y = layer_forward(leaves, leaves["x"], nhead, window, alpha, eps, dtype)
    y.backward(case["dy"].to(dtype))
    out = {k: leaves[k].grad.to(F64) for k in LAYER_PARAMS}
    out.update(y=y.detach().to(F64), dx=leaves["x"].grad.to(F64))
    return out


# ---- the transformer chain ----------------------------------------------------------------------------------------------------------------------
def model_torch(params, signal, dscores, mask, convs, depth, nhead, window, alpha, upsample, scale, clamp, dtype, eps=EPS):
    """conv x n (swish) -> [N][T][C] -> TransformerEncoderLayer x depth -> LinearUpsample -> (linear) scale, clamped, restated in torch in
    `dtype` on the parameters `params` ({the encoder's parameter name: fp32 tensor}); signal fp16 [N][L]. The clamp's gradient passes
    where `mask` = [lo < scores < hi], read from the device's stored scores as in tests/train_layers_ref.py: no reference decides a mask
    of its own. convs: [(name prefix, stride, padding)]; the layers' prefixes are "transformer_encoder.<i>."; then "upsample.linear." and
    "crf.linear.". Backward with the upstream gradient dscores [N][T'][C] -> (scores, {name: gradient float64})."""
    leaves = {k: v.to(dtype).clone().requires_grad_() for k, v in params.items()}
    h = signal.to(dtype)[:, None, :]
    for prefix, stride, padding in convs:
        h = F.silu(F.conv1d(h, leaves[prefix + "conv.weight"], leaves[prefix + "conv.bias"], stride=stride, padding=padding))
    h = h.permute(0, 2, 1)
    for i in range(depth):
        h = layer_forward(leaves, h, nhead, window, alpha, eps, dtype, prefix="transformer_encoder.%d." % i)
    N, T, D = h.shape
    h = F.linear(h, leaves["upsample.linear.weight"], leaves["upsample.linear.bias"]).reshape(N, upsample * T, D)
    y = F.linear(h, leaves["crf.linear.weight"]) * scale
    y = torch.where(mask, y, y.detach().clamp(clamp[0], clamp[1]))       # the clamped value, and no gradient through it
    y.backward(dscores.to(dtype))
    return y.detach().to(F64), {k: v.grad.to(F64) for k, v in leaves.items()}


# ---- a small transformer-family model --------------------------------------------------------------------------------------------------------
MODEL = dict(d_model=128, nhead=2, dim_feedforward=256, depth=2, window=(3, 5), upsample=2, scale=5.0, clamp=(-5.0, 5.0),
             alpha=round((2 * 2) ** 0.25, 7), beta=round((8 * 2) ** (-1 / 4), 7),         # deepnorm_params(2)
             convs=(("conv.0.", 1, 2), ("conv.1.", 1, 2), ("conv.2.", 3, 4)))            # (prefix, stride, padding)


def model_config(norm=None, time_major=False):
    """The config (a plain dict, as load_toml returns it) of convs 1 -> 16 -> 32 -> 128 (the last with stride 3), permute [0,2,1], two
    encoder layers, upsample x2, a linear CRF head (state_len 3, scale 5, blank_score 2) and clamp +-5: the v5 `sup` stack in small.
    `norm`: on every convolution. `time_major`: permute [2,0,1] instead, the LSTM family's arrangement."""
    m = MODEL
    conv = lambda i, o, k, s=1: dict(type="convolution", insize=i, size=o, winlen=k, stride=s, padding=k // 2, bias=True, activation="swish",   # noqa: E731
                                     **({"norm": norm} if norm else {}))
    layer = dict(type="transformerencoderlayer", d_model=m["d_model"], nhead=m["nhead"], dim_feedforward=m["dim_feedforward"],
                 deepnorm_alpha=m["alpha"], deepnorm_beta=m["beta"], attn_window=list(m["window"]))
    encoder = {"type": "namedserial",
               "conv": {"type": "serial", "sublayers": [conv(1, 16, 5), conv(16, 32, 5), conv(32, m["d_model"], 9, 3),
                                                        {"type": "permute", "dims": [2, 0, 1] if time_major else [0, 2, 1]}]},
               "transformer_encoder": {"type": "stack", "depth": m["depth"], "layer": layer},
               "upsample": {"type": "linearupsample", "d_model": m["d_model"], "scale_factor": m["upsample"]},
               "crf": {"type": "linearcrfencoder", "insize": m["d_model"], "n_base": 4, "state_len": 3, "bias": False, "scale": m["scale"],
                       "blank_score": 2.0, "expand_blanks": True, "permute": [1, 0, 2]},
               "clamp": {"type": "clamp", "min": m["clamp"][0], "max": m["clamp"][1]}}
    return {"model": {"type": "seqdistmodel", "package": "bonito.transformer", "seqdist": {"state_len": 3, "alphabet": ["N", "A", "C", "G", "T"]},
                      "encoder": encoder}}


def model_batch(N, L=240, seed=3):
    """-> (x fp16 [N][1][L], targets int64 [N][8], lengths [N]): 4..8 bases per chunk."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, 1, L, generator=g).half()
    lengths = torch.randint(4, 9, (N,), generator=g)
    targets = torch.zeros(N, 8, dtype=torch.int64)
    for n in range(N):
        targets[n, :lengths[n]] = torch.randint(1, 5, (int(lengths[n]),), generator=g)
    return x, targets, lengths

"""References of batch-statistics BatchNorm behind a convolution (bh_batchnorm_train_*, bonito_amd.train_ops.batchnorm,
SeqdistModel.forward_train(norm="batch")): the references of tests/test_gpu_batchnorm_train.py and tests/test_gpu_batchnorm_train_model.py,
pinned by tests/test_batchnorm_train_ref_cpu.py. Plain torch on the CPU; no import of bonito_amd.

    y = clamp(act(gamma (z - mean_c) rstd_c + beta), lo, hi)      z [N][L][C] channel-minor, statistics over the M = N L rows

As in train_layers_ref.py every reference takes the clamp's mask m = [lo < y < hi] as an INPUT (the device defines it on its stored fp16
y), so that no reference decides a mask of its own.

    formulas    the written-out forward, backward and running-statistics update, in fp64
    exact       fp64 torch: F.batch_norm(training=True) + activation under autograd, on the fp16-rounded z and dy and the fp32 gamma, beta
    yardstick   the same in fp16 on the CPU: how far half-precision training is from `exact` on a given case
    emulate     an fp32 statement of the device's design: fp32 sums of row blocks added in block order, the CENTRED second pass, fp16 y
                and dz, the mask from its own fp16 y; with `defect` one planted mistake

dist(a, exact) = max|a - exact| / max|exact| in fp64. y, dz, dgamma, dbeta must satisfy dist(kernel) <= 2 dist(yardstick).

mean, rstd, running_mean and running_var are fp32 on the device and are held against fp64 within stat_bounds(): a bound DERIVED from
the order of summation, a formula in M and the rows of a partial sum, not a tuned constant (see depth()).
"""
import math

import torch
import torch.nn.functional as F

from train_layers_ref import act_fn, act_grad, dist, mask_of  # noqa: F401  (one definition of each)

F64 = torch.float64
MARGIN = 2.0
EPS = 1e-5
MOMENTUM = 0.1
CLAMP = (-0.25, 0.75)      # both bounds bite behind a normalisation: swish goes down to -0.28, tanh up to 1
NAMES = ("y", "dz", "dgamma", "dbeta")
STATS = ("mean", "rstd", "running_mean", "running_var")
DEFECTS = ("biased_running_var", "xhat_term_dropped", "dbeta_term_dropped", "M_taken_as_L", "eps_missing", "act_grad_at_z",
           "gamma_missing_from_dz", "raw_moments")
U32 = 2.0 ** -24          # unit roundoff of fp32

# the split of the rows, csrc/batchnorm_train.hip: blocks of at least MIN_ROWS rows, at most MAX_BLOCKS of them; 256 threads per block
MIN_ROWS, MAX_BLOCKS, THREADS, RUNS = 64, 2048, 256, 8


def block_rows(M):
    return max(MIN_ROWS, -(-M // MAX_BLOCKS))


def depth(M):
    """An upper bound of the number of fp32 additions any single value passes through on its way into a per-channel sum: a thread
    adds at most block_rows(M) rows in row order, the at most 256 row slots of a workgroup are added in slot order, and the B blocks in
    RUNS runs of ceil(B / RUNS) blocks followed by the RUNS runs. A sum of n terms added in ANY fixed order of depth d has the error
    |fl(sum) - sum| <= d u sum|x_i| to first order in u (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2)."""
    P = block_rows(M)
    B = -(-M // P)
    return P + THREADS + -(-B // RUNS) + RUNS


def stat_bounds(z, running_mean, running_var, eps=EPS, momentum=MOMENTUM):
    """Per-channel absolute bounds {name: fp64 [C]} on the device's fp32 statistics against fp64, from the order of summation.
        mean: the sum of the fp16 values (exact in fp32) has depth d, then one division: (d + 1) u mean|z|.
        var:  sum (z - mean')^2 = sum (z - mean)^2 + M (mean' - mean)^2 exactly, every term is rounded three times (difference, square,
              fused add: <= 3 u relative) and the non-negative terms are summed at depth d, one division: (d + 4) u (var + dm^2) + dm^2
              with dm the bound of the mean.
        rstd = (var + eps)^-1/2: the derivative is rstd / (2 (var + eps)); the addition, the square root and the division round: 3 u.
        running statistics: the linear map of the two, its two products and one sum rounded (<= 3 u of the magnitudes); the unbiased
              factor M / (M - 1) is formed and applied in fp32 (2 u more)."""
    zf = z.to(F64).reshape(-1, z.shape[-1])
    M = zf.shape[0]
    d = depth(M)
    mean, var = zf.mean(0), zf.var(0, unbiased=False)
    dm = (d + 1) * U32 * zf.abs().mean(0)
    dv = (d + 4) * U32 * (var + dm * dm) + dm * dm
    rstd = (var + eps).rsqrt()
    out = {"mean": dm, "rstd": rstd * (0.5 * dv / (var + eps) + 3 * U32)}
    if running_mean is not None:
        unb = var * M / (M - 1)
        out["running_mean"] = momentum * dm + 3 * U32 * (running_mean.to(F64).abs() + mean.abs())
        out["running_var"] = momentum * (dv * M / (M - 1)) + 5 * U32 * (running_var.to(F64).abs() + unb)
    return out


def bn_case(N, L, C, seed=0, offset_channel=None, constant_channel=None):
    """-> {z fp16 [N][L][C], gamma, beta fp32 [C], dy fp16 [N][L][C] (mean 0.5: a gradient whose channel sums do not vanish),
    running_mean, running_var fp32 [C]}. Seeded. offset_channel: mean 8,
    standard deviation 0.05 (where E[z^2] - E[z]^2 in fp32 has no digit left); constant_channel: one value throughout (variance 0)."""
    g = torch.Generator().manual_seed(9700 + seed + 31 * C + 7 * L + N)
    z = torch.randn(N, L, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + torch.randn(C, generator=g)
    if offset_channel is not None:
        z[:, :, offset_channel] = 8.0 + 0.05 * torch.randn(N, L, generator=g)
    if constant_channel is not None:
        z[:, :, constant_channel] = 1.375
    return {"z": z.half(), "gamma": 1.0 + 0.3 * torch.randn(C, generator=g), "beta": 0.3 * torch.randn(C, generator=g),
            "dy": (0.5 + torch.randn(N, L, C, generator=g)).half(), "running_mean": torch.randn(C, generator=g),
            "running_var": 0.5 + torch.rand(C, generator=g)}


def _affine(case, C, dtype):
    gamma = case.get("gamma")
    if gamma is None:
        return torch.ones(C, dtype=dtype), torch.zeros(C, dtype=dtype)
    return gamma.to(dtype), case["beta"].to(dtype)


def formulas(case, act, m, eps=EPS, momentum=MOMENTUM):
    """The layer written out in fp64 -> {y, dz, dgamma, dbeta, mean, rstd, running_mean, running_var} (the clamp is the mask m)."""
    z, dy = case["z"].to(F64), case["dy"].to(F64)
    C = z.shape[-1]
    M = z.numel() // C
    gamma, beta = _affine(case, C, F64)
    mean = z.reshape(M, C).sum(0) / M
    var = ((z - mean) ** 2).reshape(M, C).sum(0) / M
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (z - mean) * rstd
    u = gamma * xh + beta
    du = dy * m.to(F64) * act_grad(u, act)
    dbeta, dgamma = du.reshape(M, C).sum(0), (du * xh).reshape(M, C).sum(0)
    out = {"y": act_fn(u, act) * m.to(F64), "dz": gamma * rstd * (du - dbeta / M - xh * dgamma / M), "dgamma": dgamma, "dbeta": dbeta,
           "mean": mean, "rstd": rstd}
    if case.get("running_mean") is not None:
        out["running_mean"] = (1 - momentum) * case["running_mean"].to(F64) + momentum * mean
        out["running_var"] = (1 - momentum) * case["running_var"].to(F64) + momentum * var * M / (M - 1)
    return out


def bn_torch(case, act, m, eps=EPS, momentum=MOMENTUM, dtype=F64):
    """torch's own batch norm in training mode + activation under autograd, in `dtype` -> the outputs of formulas() in fp64 (mean and
    rstd are not torch's to give: they are left out)."""
    z = case["z"].to(dtype).clone().requires_grad_()
    C = z.shape[-1]
    affine = case.get("gamma") is not None
    gamma, beta = (t.clone().requires_grad_() for t in _affine(case, C, dtype))
    tracked = case.get("running_mean") is not None
    rm = case["running_mean"].to(dtype).clone() if tracked else None
    rv = case["running_var"].to(dtype).clone() if tracked else None
    zc = z.permute(0, 2, 1)                                                                     # torch normalises dim 1
    u = F.batch_norm(zc, rm, rv, gamma if affine else None, beta if affine else None, True, momentum, eps).permute(0, 2, 1)
    y = act_fn(u, act) * m.to(dtype)
    y.backward(case["dy"].to(dtype))
    out = {"y": y.detach().to(F64), "dz": z.grad.to(F64), "dgamma": gamma.grad.to(F64) if affine else None,
           "dbeta": beta.grad.to(F64) if affine else None}
    if tracked:
        out["running_mean"], out["running_var"] = rm.to(F64), rv.to(F64)
    return out


def exact(case, act, m, eps=EPS, momentum=MOMENTUM):
    return bn_torch(case, act, m, eps, momentum, F64)


def yardstick(case, act, m, eps=EPS, momentum=MOMENTUM):
    return bn_torch({k: None if v is None else v.cpu() for k, v in case.items()}, act, m.cpu(), eps, momentum, torch.float16)


def _block_sum(rows):
    """fp32 sums of [M][C] rows: the blocks of block_rows(M) rows, each summed in fp32, added in block order."""
    P = block_rows(rows.shape[0])
    total = torch.zeros(rows.shape[1], dtype=torch.float32)
    for lo in range(0, rows.shape[0], P):
        total = total + rows[lo:lo + P].sum(0, dtype=torch.float32)
    return total


def emulate(case, act, clamp, eps=EPS, momentum=MOMENTUM, defect=None):
    """The device's design in fp32 -> (m bool, {y fp16, dz fp16, dgamma, dbeta, mean, rstd fp32, running_mean, running_var fp32})."""
    f32 = torch.float32
    z, dy = case["z"].float(), case["dy"].float()
    N, L, C = z.shape
    M = L if defect == "M_taken_as_L" else N * L
    gamma, beta = _affine(case, C, f32)
    rows = z.reshape(-1, C)
    mean = _block_sum(rows) / M
    if defect == "raw_moments":
        var = _block_sum(rows * rows) / M - mean * mean
    else:
        var = _block_sum((rows - mean) ** 2) / M
    rstd = 1.0 / torch.sqrt(var if defect == "eps_missing" else var + f32_(eps))
    xh = (z - mean) * rstd
    u = gamma * xh + beta
    a = act_fn(u, act)
    y16 = (a if clamp is None else a.clamp(clamp[0], clamp[1])).half()
    m = mask_of(y16, clamp)
    du = dy * m * act_grad(z if defect == "act_grad_at_z" else u, act)
    dbeta, dgamma = _block_sum(du.reshape(-1, C)), _block_sum((du * xh).reshape(-1, C))
    inner = du - (0.0 if defect == "dbeta_term_dropped" else dbeta / M) - (0.0 if defect == "xhat_term_dropped" else xh * dgamma / M)
    dz = ((1.0 if defect == "gamma_missing_from_dz" else gamma) * rstd * inner).half()
    out = {"y": y16, "dz": dz, "dgamma": dgamma, "dbeta": dbeta, "mean": mean, "rstd": rstd}
    if case.get("running_mean") is not None:
        unbiased = var if defect == "biased_running_var" else var * (f32_(M) / f32_(M - 1))
        out["running_mean"] = (1 - f32_(momentum)) * case["running_mean"] + f32_(momentum) * mean
        out["running_var"] = (1 - f32_(momentum)) * case["running_var"] + f32_(momentum) * unbiased
    assert all(v.dtype in (torch.float16, f32) for v in out.values())
    return m, out


def f32_(v):
    return torch.tensor(float(v), dtype=torch.float32)


def outside(got, want, yard, bounds, m, names=NAMES, stats=STATS):
    """The names of the outputs of `got` that miss their check against `want` (fp64): 2 dist(yardstick) for the layer's outputs, the
    derived bound for the statistics. Outputs that `want` does not hold (None) are passed over. y is compared where the mask m holds:
    the references multiply by m where the device clamps (outside m the device's y is the bound itself, which its tests assert)."""
    bad = []
    for name in names:
        g = got[name] * m.to(got[name].device) if name == "y" else got[name]
        if want.get(name) is not None and not dist(g, want[name]) <= MARGIN * dist(yard[name], want[name]):
            bad.append(name)
    for name in stats:
        if want.get(name) is not None and name in bounds:
            err = (got[name].to(F64).cpu() - want[name].to(F64)).abs()
            if not bool((err <= bounds[name]).all()):
                bad.append(name)
    return bad


# ---- the models of tests/test_gpu_batchnorm_train_model.py ------------------------------------------------------------------------------------
LSTM_CONVS = (("0.", 1, 2), ("1.", 1, 2), ("2.", 5, 9))            # (prefix, stride, padding)
LSTM_LAYERS = (("4.", True), ("5.", False), ("6.", True), ("7.", False), ("8.", True))        # (prefix, reverse)
HEAD, SCALE = "9.", 5.0


def lstm_config():
    """The 32-feature model of tests/test_gpu_train_model.py (convolutions 1 -> 4 -> 16 -> 32, the 4 channels served by zero padding;
    five LSTM layers; a tanh head with scale 5) as a new-style config whose convolutions carry norm = "batchnorm", as every published
    configuration does. Its parameters in train_layers_ref.chain_params' order: lstm_model_names()."""
    conv = lambda i, o, k, s: {"type": "convolution", "insize": i, "size": o, "bias": True, "winlen": k, "stride": s, "padding": k // 2,      # noqa: E731
                               "activation": "swish", "norm": "batchnorm"}
    lstm = lambda rev: {"type": "lstm", "size": 32, "insize": 32, "bias": True, "reverse": rev}                                       # noqa: E731
    return {"model": {"package": "bonito_amd.crf"},
            "labels": {"labels": ["N", "A", "C", "G", "T"]},
            "input": {"features": 1},
            "global_norm": {"state_len": 3},
            "encoder": {"type": "serial", "sublayers": [
                conv(1, 4, 5, 1), conv(4, 16, 5, 1), conv(16, 32, 19, 5), {"type": "permute", "dims": [2, 0, 1]}]
                + [lstm(rev) for _, rev in LSTM_LAYERS]
                + [{"type": "linearcrfencoder", "insize": 32, "n_base": 4, "state_len": 3, "bias": True, "scale": SCALE, "activation": "tanh",
                    "blank_score": 2.0, "expand_blanks": True, "permute": [1, 0, 2]}]}}


def misbuilt_models():
    """-> [(name, model, the refusal forward_train(x, norm="batch") owes it)]: five encoders that begin with a normalised convolution
    and are wrong further on, in ways only the layout the activations have at a layer can tell. A refusal that came after the first
    layer had run would have rewritten that convolution's BatchNorm buffers. x is [2, 1, 120]."""
    from bonito_amd import nn as bnn
    from bonito_amd.crf.model import CTC_CRF, SeqdistModel

    def conv():
        return bnn.Convolution(1, 32, 5, padding=2, activation="swish", norm="batchnorm")

    def head():
        return bnn.LinearCRFEncoder(32, 4, 3, blank_score=2.0)

    encoders = (
        ("no head", [conv(), bnn.Permute([2, 0, 1]), bnn.LSTM(32, 32)], "the encoder does not end in a linearcrfencoder"),
        ("lstm without permute", [conv(), bnn.LSTM(32, 32), head()], r"layer 1 \(LSTM\) must follow permute \[2,0,1\]"),
        ("conv after permute", [conv(), bnn.Permute([2, 0, 1]), bnn.Convolution(32, 32, 5, padding=2), head()],
         r"layer 2 \(Convolution\) follows the permute to time-major activations"),
        ("stray clamp", [conv(), bnn.Permute([2, 0, 1]), bnn.Clamp(-1, 1), bnn.LSTM(32, 32), head()],
         r"layer 2 \(Clamp\) follows no convolution, linear or head to be fused into"),
        ("second conv of one channel", [conv(), bnn.Convolution(1, 32, 5, padding=2), bnn.Permute([2, 0, 1]), bnn.LSTM(32, 32), head()],
         r"layer 1 \(Convolution\) expects 1 input channels"))
    return [(name, SeqdistModel(bnn.Serial(layers), CTC_CRF(3, ["N", "A", "C", "G", "T"])).train(), text) for name, layers, text in encoders]


def batchnorm_buffers(model):
    """Copies of running_mean, running_var and num_batches_tracked of every BatchNorm in the model."""
    return {k: v.detach().clone() for k, v in model.named_buffers() if k.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked")}


def lstm_model_names():
    """The encoder's parameter names in the order of train_layers_ref.chain_params(32, 4, 5, 19, 5, 256)."""
    names = [p + "conv." + k for p, _, _ in LSTM_CONVS for k in ("weight", "bias")]
    names += [p + "rnn." + k for p, _ in LSTM_LAYERS for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0")]
    return names + [HEAD + "linear.weight", HEAD + "linear.bias"]


def _leaves(params, dtype):
    """The encoder's parameters as torch leaves in `dtype`: the fp16-rounded values of what the device rounds (convolution, LSTM and
    linear weights and biases), the values as they are of what it uses unrounded (every norm's parameters)."""
    return {k: (v if "norm" in k else v.half()).to(dtype).clone().requires_grad_() for k, v in params.items()}


def _convs(leaves, buffers, h, convs, training):
    """conv -> torch's batch norm (training: batch statistics, and `buffers` are updated in place as torch does) -> swish, [N][C][L]."""
    # A bias in front of a batch norm has the gradient sum_m dz = 0 identically: a relative distance from it is 0 / 0. What the device
    # returns there is the rounding of its fp16 dz (fp32 sums of values rounded once, 2^-11 relative): |db_c| <= 2^-11 sum_m |dz_mc|.
    for prefix, stride, padding in convs:
        h = F.conv1d(h, leaves[prefix + "conv.weight"], leaves[prefix + "conv.bias"], stride=stride, padding=padding)
        if h.requires_grad:                 # d loss / d z [N][C][L] is handed out beside the parameters' gradients, as "<prefix>conv.z"
            h.retain_grad()
            leaves[prefix + "conv.z"] = h
        h = F.silu(F.batch_norm(h, buffers[prefix + "norm.bn.running_mean"], buffers[prefix + "norm.bn.running_var"],
                                leaves[prefix + "norm.bn.weight"], leaves[prefix + "norm.bn.bias"], training, MOMENTUM, EPS))
    return h


def _finish(y, leaves, buffers, dscores, dtype):
    if dscores is not None:
        y.backward(dscores.to(dtype))
    return y.detach().to(F64), {k: v.grad.to(F64) for k, v in leaves.items() if v.grad is not None}, {k: v.to(F64) for k, v in buffers.items()}


def lstm_model_torch(params, buffers, signal, dscores=None, dtype=F64, training=True):
    """The encoder of lstm_config() restated in torch in `dtype`: signal fp16 [N][L] -> scores [N][T][256]; params / buffers: the
    encoder's named_parameters / named_buffers (CPU). -> (scores, {name: gradient} for the upstream gradient dscores, the buffers
    after the call), all float64. bias_hh_l0 is zero in these models and not read."""
    from train_layers_ref import lstm_layer
    leaves = _leaves(params, dtype)
    buffers = {k: v.to(dtype).clone() for k, v in buffers.items() if v.is_floating_point()}
    h = _convs(leaves, buffers, signal.to(dtype)[:, None, :], LSTM_CONVS, training).permute(2, 0, 1)
    for prefix, reverse in LSTM_LAYERS:
        h = lstm_layer(h, leaves[prefix + "rnn.weight_ih_l0"], leaves[prefix + "rnn.weight_hh_l0"], leaves[prefix + "rnn.bias_ih_l0"], reverse)
    y = (torch.tanh(F.linear(h, leaves[HEAD + "linear.weight"], leaves[HEAD + "linear.bias"])) * SCALE).permute(1, 0, 2)
    return _finish(y, leaves, buffers, dscores, dtype)


def v5_model_torch(params, buffers, signal, mask, dscores=None, dtype=F64, training=True):
    """The encoder of transformer_train_ref.model_config(norm="batchnorm") restated in torch: its model_torch with the batch norm
    between each convolution and its swish. mask = [lo < scores < hi] read from the device's stored scores."""
    import transformer_train_ref as tt
    m = tt.MODEL
    leaves = _leaves(params, dtype)
    buffers = {k: v.to(dtype).clone() for k, v in buffers.items() if v.is_floating_point()}
    h = _convs(leaves, buffers, signal.to(dtype)[:, None, :], m["convs"], training).permute(0, 2, 1)
    for i in range(m["depth"]):
        h = tt.layer_forward(leaves, h, m["nhead"], m["window"], m["alpha"], tt.EPS, dtype, prefix="transformer_encoder.%d." % i)
    N, T, D = h.shape
    h = F.linear(h, leaves["upsample.linear.weight"], leaves["upsample.linear.bias"]).reshape(N, m["upsample"] * T, D)
    y = F.linear(h, leaves["crf.linear.weight"]) * m["scale"]
    y = torch.where(mask, y, y.detach().clamp(m["clamp"][0], m["clamp"][1]))       # the clamped value, and no gradient through it
    return _finish(y, leaves, buffers, dscores, dtype)

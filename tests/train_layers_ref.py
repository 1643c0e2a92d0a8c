"""References of the training convolution and linear / CRF-head layer (bh_conv1d_train_*, bh_linear_train_*, bonito_amd.train_ops) and
of the chain SeqdistModel.forward_train builds: the references of tests/test_gpu_train_layers.py and tests/test_gpu_train_model.py,
pinned by tests/test_train_layers_ref_cpu.py. Plain torch on the CPU; no import of bonito_amd.

    convolution   y = clamp(act(conv(x, W) + b), lo, hi)      x [N][Lin][Cin] channel-minor, y [N][Lout][Cout]
    linear        Y = clamp(act(X W^T + b) scale, lo, hi)     X [T][N][K], Y [T][N][C]

Every reference takes the clamp's mask m = [lo < y < hi] as an INPUT (the device defines it on its stored fp16 y): the clamp is replaced
by a multiplication with m, so that no reference decides a mask of its own.

    exact       fp64 torch autograd of the layer on the fp16-rounded inputs: what the kernels are measured against
    yardstick   the same in fp16 on the CPU (F.conv1d, F.silu, F.linear, torch.tanh on .half() tensors): how far half-precision
                training is from `exact` on a given case
    emulate     an fp32 statement of the device's design: dz rounded to fp16, fp32 sums, dx rounded to fp16, the mask from its own fp16 y,
                tanh' from the stored Y; with `defect` one planted mistake

dist(a, exact) = max|a - exact| / max|exact| in fp64. The device tests require dist(kernel) <= 2 dist(yardstick) per gradient.
"""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64
MARGIN = 2.0
CLAMP = (-0.5, 3.5)

# (N, Cin, Cout, K, stride, Lin), swish, padding K // 2
CONV_CASES = ((3, 1, 4, 5, 1, 203), (2, 1, 16, 5, 1, 67), (3, 4, 16, 5, 1, 200), (3, 16, 16, 5, 1, 203), (3, 16, 96, 19, 5, 403),
              (2, 16, 384, 19, 6, 401), (5, 16, 32, 19, 5, 90), (1, 16, 1024, 19, 5, 35))
# (T, N, K, C, act, scale, clamp, bias)
LINEAR_CASES = ((20, 3, 96, 1024, "tanh", 5.0, None, True), (9, 5, 32, 80, "tanh", 5.0, None, True), (16, 4, 384, 320, "tanh", 5.0, None, False),
                (7, 5, 64, 256, None, None, (-5.0, 5.0), False), (33, 4, 128, 64, None, None, None, True), (3, 9, 1024, 256, None, None, None, True))
CONV_DEFECTS = ("tap_off_by_one", "stride_on_tap", "padding_off_by_one", "mask_inclusive", "last_row_block_dropped", "bias_wrong_axis")
LINEAR_DEFECTS = ("scale_omitted", "dx_through_w", "mask_inclusive", "last_row_block_dropped", "bias_wrong_axis")
ROW_BLOCK = 32      # rows of one MFMA of the reduction over rows


def dist(a, want):
    """max|a - want| / max|want| in fp64 (0 / 0 = 0; a non-finite a is inf)."""
    a, want = a.detach().to(F64).cpu(), want.detach().to(F64).cpu()
    if not bool(torch.isfinite(a).all()):
        return float("inf")
    err, ref = float((a - want).abs().max()), float(want.abs().max())
    return 0.0 if err == 0.0 else err / ref if ref > 0 else float("inf")


def conv_out_len(Lin, K, stride, pad):
    return (Lin + 2 * pad - K) // stride + 1


def act_fn(z, act):
    if act == "swish":
        return F.silu(z)
    if act == "tanh":
        return torch.tanh(z)
    if act == "relu":
        return torch.relu(z)
    return z


def act_grad(z, act):
    if act == "swish":
        s = torch.sigmoid(z)
        return s * (1 + z * (1 - s))
    if act == "tanh":
        return 1 - torch.tanh(z) ** 2
    if act == "relu":
        return (z > 0).to(z.dtype)
    return torch.ones_like(z)


def mask_of(y16, clamp, inclusive=False):
    """[lo < y < hi] on stored fp16 values (all ones without a clamp)."""
    if clamp is None:
        return torch.ones(y16.shape, dtype=torch.bool, device=y16.device)
    y = y16.float()
    return ((y >= clamp[0]) & (y <= clamp[1])) if inclusive else ((y > clamp[0]) & (y < clamp[1]))


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def conv_inputs(case, scale=1.0, seed=0):
    """-> x fp16 [N][Lin][Cin], w fp32 [Cout][Cin][K], b fp32 [Cout], dy fp16 [N][Lout][Cout], padding. Seeded; x ~ scale N(0, 1)."""
    N, Cin, Cout, K, stride, Lin = case
    g = torch.Generator().manual_seed(9100 + seed + 17 * Cout + Lin)
    pad = K // 2
    x = (torch.randn(N, Lin, Cin, generator=g) * scale).half()
    w = torch.randn(Cout, Cin, K, generator=g) / math.sqrt(Cin * K)
    b = torch.randn(Cout, generator=g) * 0.1
    dy = torch.randn(N, conv_out_len(Lin, K, stride, pad), Cout, generator=g).half()
    return x, w, b, dy, pad


def linear_inputs(case, seed=0):
    """-> x fp16 [T][N][K], w fp32 [C][K], b fp32 [C] or None, dy fp16 [T][N][C]."""
    T, N, K, C, act, scale, clamp, bias = case
    g = torch.Generator().manual_seed(9300 + seed + 13 * C + K)
    x = torch.randn(T, N, K, generator=g).half()
    gain = 1.0 if act == "tanh" else 3.0            # the clamped case needs outputs on both sides of +-5
    w = torch.randn(C, K, generator=g) * (gain / math.sqrt(K))
    b = torch.randn(C, generator=g) * 0.1 if bias else None
    dy = torch.randn(T, N, C, generator=g).half()
    return x, w, b, dy


# ---- convolution ------------------------------------------------------------------------------------------------------------------------
def conv_ref(x, w, b, m, dy, stride, pad, act, dtype):
    """torch autograd in `dtype` on the fp16-rounded inputs -> {dx [N][Lin][Cin], dw, db (or None)} float64."""
    xd = x.half().to(dtype).clone().requires_grad_()
    wd = w.half().to(dtype).clone().requires_grad_()
    bd = None if b is None else b.half().to(dtype).clone().requires_grad_()
    z = F.conv1d(xd.permute(0, 2, 1), wd, bd, stride=stride, padding=pad)
    y = act_fn(z, act).permute(0, 2, 1) * m.to(dtype)
    y.backward(dy.to(dtype))
    return {"dx": xd.grad.to(F64), "dw": wd.grad.to(F64), "db": None if b is None else bd.grad.to(F64)}


def conv_exact(x, w, b, m, dy, stride, pad, act):
    return conv_ref(x, w, b, m, dy, stride, pad, act, F64)


def conv_yardstick(x, w, b, m, dy, stride, pad, act):
    return conv_ref(x.cpu(), w.cpu(), None if b is None else b.cpu(), m.cpu(), dy.cpu(), stride, pad, act, torch.float16)


def _windows(xf, K, stride, pad, Lout, tap_stride=1, pos_stride=None):
    """[N][Lout][Cin][K]: element (t, k) = x[t * pos_stride - pad + k * tap_stride], zero outside."""
    N, Lin, Cin = xf.shape
    pos_stride = stride if pos_stride is None else pos_stride
    t = torch.arange(Lout)[:, None] * pos_stride - pad + torch.arange(K)[None, :] * tap_stride       # [Lout][K]
    ok = (t >= 0) & (t < Lin)
    win = xf[:, t.clamp(0, Lin - 1)]                                                                 # [N][Lout][K][Cin]
    return (win * ok[None, :, :, None]).permute(0, 1, 3, 2)


def conv_emulate(x, w, b, dy, stride, pad, act, clamp, defect=None):
    """The device's design in fp32 -> (y fp16, m bool, {dx fp16, dw fp32, db fp32})."""
    xf, wf = x.half().float(), w.half().float()
    bf = torch.zeros(w.shape[0]) if b is None else b.half().float()
    N, Lin, Cin = xf.shape
    Cout, _, K = wf.shape
    Lout = conv_out_len(Lin, K, stride, pad)
    win = _windows(xf, K, stride, pad, Lout)
    z = torch.einsum("nlck,ock->nlo", win, wf) + bf
    a = act_fn(z, act)
    y16 = (a if clamp is None else a.clamp(clamp[0], clamp[1])).half()
    m = mask_of(y16, clamp)
    used = mask_of(y16, clamp, inclusive=True) if defect == "mask_inclusive" else m
    dz = (dy.float() * act_grad(z, act) * used).half().float()
    gwin = win
    if defect == "tap_off_by_one":
        gwin = _windows(xf, K, stride, pad - 1, Lout)
    elif defect == "stride_on_tap":
        gwin = _windows(xf, K, stride, pad, Lout, tap_stride=stride, pos_stride=1)
    elif defect == "padding_off_by_one":
        gwin = _windows(xf, K, stride, pad + 1, Lout)
    rows = dz.reshape(-1, Cout)
    rwin = gwin.reshape(-1, Cin, K)
    if defect == "last_row_block_dropped":
        keep = (rows.shape[0] - 1) // ROW_BLOCK * ROW_BLOCK
        rows, rwin = rows[:keep], rwin[:keep]
    dw = torch.einsum("mo,mck->ock", rows, rwin)
    db = rows.sum(0)
    if defect == "bias_wrong_axis":
        db = dz.reshape(-1)[:dz.numel() // Cout * Cout].reshape(Cout, -1).sum(1)
    gpad = pad + 1 if defect == "padding_off_by_one" else pad - 1 if defect == "tap_off_by_one" else pad
    dxp = torch.zeros(N, Lin + 2 * (pad + 1) + K * stride, Cin)
    off = pad + 1                                                  # dxp index = input position + off
    for k in range(K):
        g = torch.einsum("nlo,oc->nlc", dz, wf[:, :, k])
        if defect == "stride_on_tap":
            start, step = off - gpad + k * stride, 1
        else:
            start, step = off - gpad + k, stride
        dxp[:, start:start + (Lout - 1) * step + 1:step] += g
    dx = dxp[:, off:off + Lin].half()
    return y16, m, {"dx": dx, "dw": dw, "db": None if b is None else db}


# ---- linear -----------------------------------------------------------------------------------------------------------------------------
def linear_ref(x, w, b, m, dy, act, scale, dtype):
    xd = x.half().to(dtype).clone().requires_grad_()
    wd = w.half().to(dtype).clone().requires_grad_()
    bd = None if b is None else b.half().to(dtype).clone().requires_grad_()
    y = act_fn(F.linear(xd, wd, bd), act)
    if scale is not None:
        y = y * scale
    (y * m.to(dtype)).backward(dy.to(dtype))
    return {"dx": xd.grad.to(F64), "dw": wd.grad.to(F64), "db": None if b is None else bd.grad.to(F64)}


def linear_exact(x, w, b, m, dy, act, scale):
    return linear_ref(x, w, b, m, dy, act, scale, F64)


def linear_yardstick(x, w, b, m, dy, act, scale):
    return linear_ref(x.cpu(), w.cpu(), None if b is None else b.cpu(), m.cpu(), dy.cpu(), act, scale, torch.float16)


def linear_emulate(x, w, b, dy, act, scale, clamp, defect=None):
    """The device's design in fp32, tanh' from the stored Y -> (y fp16 [T][N][C], m bool, {dx fp16, dw fp32, db fp32})."""
    xf, wf = x.half().float(), w.half().float()
    T, N, K = xf.shape
    C = wf.shape[0]
    s = 1.0 if scale is None else float(scale)
    z = xf.reshape(-1, K) @ wf.T
    if b is not None:
        z = z + b.half().float()
    a = act_fn(z, act) * s
    y16 = (a if clamp is None else a.clamp(clamp[0], clamp[1])).half()
    m = mask_of(y16, clamp)
    used = mask_of(y16, clamp, inclusive=True) if defect == "mask_inclusive" else m
    g = torch.full_like(z, 1.0 if defect == "scale_omitted" else s)
    if act == "tanh":
        g = g * (1 - (y16.float() / s) ** 2)
    dz = (dy.float().reshape(-1, C) * g * used).half().float()
    dx = (dz @ (wf.T.reshape(C, K) if defect == "dx_through_w" else wf)).half().reshape(T, N, K)
    rows, rx = dz, xf.reshape(-1, K)
    if defect == "last_row_block_dropped":
        keep = (rows.shape[0] - 1) // ROW_BLOCK * ROW_BLOCK
        rows, rx = rows[:keep], rx[:keep]
    dw = rows.T @ rx
    db = rows.sum(0)
    if defect == "bias_wrong_axis":
        db = dz.reshape(-1)[:dz.numel() // C * C].reshape(C, -1).sum(1)
    return y16.reshape(T, N, C), m.reshape(T, N, C), {"dx": dx, "dw": dw, "db": None if b is None else db}


# ---- the chain of an old-style rnn_encoder model (no clamps, no norm) ------------------------------------------------------------------
def lstm_layer(x, w_ih, w_hh, bias, reverse):
    """x [T][N][H] -> h [T][N][H]; gates i, f, g, o; h_0 = c_0 = 0; in x's dtype."""
    T, N, H = x.shape
    xs = x.flip(0) if reverse else x
    proj = xs @ w_ih.T + (bias if bias is not None else 0)
    h = torch.zeros(N, H, dtype=x.dtype)
    c = torch.zeros(N, H, dtype=x.dtype)
    out = []
    for t in range(T):
        ai, af, ag, ao = (proj[t] + h @ w_hh.T).split(H, dim=-1)
        c = torch.sigmoid(af) * c + torch.sigmoid(ai) * torch.tanh(ag)
        h = torch.sigmoid(ao) * torch.tanh(c)
        out.append(h)
    hs = torch.stack(out)
    return hs.flip(0) if reverse else hs


class _Round16(torch.autograd.Function):
    """Round to fp16 values on the way forward, and the gradient on the way back: what storing an activation and its gradient as fp16 does."""

    @staticmethod
    def forward(ctx, t):
        return t.half().to(t.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.half().to(g.dtype)


def chain_params(features, first_conv, stride, winlen, n_layers, n_out, seed=0):
    """fp32 parameters of conv x3 -> LSTM x n -> tanh head, in the order of the encoder's named_parameters: list of (name, tensor)."""
    g = torch.Generator().manual_seed(9500 + seed)
    r = lambda *s, gain=1.0: torch.randn(*s, generator=g) * gain      # noqa: E731
    p = [("conv0.weight", r(first_conv, 1, 5, gain=1 / math.sqrt(5))), ("conv0.bias", r(first_conv, gain=0.1)),
         ("conv1.weight", r(16, first_conv, 5, gain=1 / math.sqrt(5 * first_conv))), ("conv1.bias", r(16, gain=0.1)),
         ("conv2.weight", r(features, 16, winlen, gain=1 / math.sqrt(16 * winlen))), ("conv2.bias", r(features, gain=0.1))]
    for i in range(n_layers):
        p += [("lstm%d.weight_ih" % i, r(4 * features, features, gain=1 / math.sqrt(features))),
              ("lstm%d.weight_hh" % i, r(4 * features, features, gain=1 / math.sqrt(features))), ("lstm%d.bias_ih" % i, r(4 * features, gain=0.1))]
    p += [("head.weight", r(n_out, features, gain=1 / math.sqrt(features))), ("head.bias", r(n_out, gain=0.1))]
    return p


def chain_ref(signal, params, dscores, stride, n_layers, scale, dtype, emulate=False):
    """The old-style encoder restated in torch, in `dtype`, on the fp16-rounded parameters: signal fp16 [N][L] -> scores [N][T][C];
    backward with the upstream gradient dscores [N][T][C] -> {name: gradient float64}. `emulate`: with dtype float32, every
    activation and its gradient rounded to fp16 between the layers, as the device stores them."""
    leaves = {n: t.half().to(dtype).clone().requires_grad_() for n, t in params}
    rnd = _Round16.apply if emulate else (lambda t: t)
    h = signal.half().to(dtype)[:, None, :]
    for i in range(3):
        w = leaves["conv%d.weight" % i]
        h = rnd(F.silu(F.conv1d(h, w, leaves["conv%d.bias" % i], stride=stride if i == 2 else 1, padding=w.shape[2] // 2)))
    h = h.permute(2, 0, 1)
    for i in range(n_layers):
        h = rnd(lstm_layer(h, leaves["lstm%d.weight_ih" % i], leaves["lstm%d.weight_hh" % i], leaves["lstm%d.bias_ih" % i],
                           reverse=bool((n_layers - i) % 2)))
    y = rnd(torch.tanh(F.linear(h, leaves["head.weight"], leaves["head.bias"])) * scale).permute(1, 0, 2)
    y.backward(dscores.to(dtype))
    return y.detach(), {n: t.grad.to(F64) for n, t in leaves.items()}

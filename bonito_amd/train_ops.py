"""
The convolution and the linear / CRF-head layer for training on the device: forward on the rounded master weights, backward, and their
autograd (csrc/train_layers.hip; the arithmetic is stated in include/bonito_hip.h under bh_conv1d_train_forward) - the two layers a
transformer encoder layer adds, the DeepNorm residual RMSNorm and the gated input layer of the MLP (csrc/transformer_train.hip; under
bh_rmsnorm_train_backward) - and the batch-statistics BatchNorm behind a convolution (csrc/batchnorm_train.hip; under
bh_batchnorm_train_forward) - and what a QuartzNet CTC model adds: the depthwise convolution, the residual add with activation and
dropout, and the 1x1 decoder with its log-softmax (csrc/quartznet_train.hip; under bh_dwconv1d_train_backward).

    y = conv1d_forward(x, weight, bias, stride, padding, activation, clamp, time_major)     # x fp16 [N][Lin][Cin] ([N][Lin] for Cin == 1)
    dx, dw, db = conv1d_backward(x, weight, bias, y, dy, stride, padding, activation, clamp, time_major)
    y = conv1d(x, weight, bias, stride, padding, activation, clamp, time_major)             # differentiable
    y = linear_forward(x, weight, bias, activation, scale, clamp, batch_major_out)          # x fp16 [T][N][K]
    dx, dw, db = linear_backward(x, weight, y, dy, activation, scale, clamp, batch_major_out)
    y = linear(x, weight, bias, activation, scale, clamp, batch_major_out)                  # differentiable
    out = rmsnorm_residual_forward(a, x, weight, alpha, eps)                                # a, x fp16 [...][D]: rmsnorm(a + alpha x) weight
    da, dx, dw = rmsnorm_residual_backward(a, x, weight, dy, alpha, eps)
    out = rmsnorm_residual(a, x, weight, alpha, eps)                                        # differentiable
    h = gated_linear_forward(x, weight)                                                     # x fp16 [...][D], weight [2F][D] -> [...][F]
    dx, dw = gated_linear_backward(x, weight, dh)
    h = gated_linear(x, weight)                                                             # differentiable
    y, mean, rstd = batchnorm_forward(z, weight, bias, running_mean, running_var, momentum, eps, activation, clamp, time_major, channels)
    dz, dw, db = batchnorm_backward(z, weight, bias, mean, rstd, y, dy, activation, clamp, time_major, channels)
    y = batchnorm(z, weight, bias, running_mean, running_var, momentum, eps, activation, clamp, time_major, channels)    # differentiable
    y = depthwise_conv1d_forward(x, weight, padding)                                        # x fp16 [N][L][C], weight fp32 [C][1][K]
    dx, dw = depthwise_conv1d_backward(x, weight, dy, padding)
    y = depthwise_conv1d(x, weight, padding)                                                # differentiable
    y = residual_act_forward(a, b, activation, p, seed, stream_id)                          # a, b fp16 [...][C]; b may be None
    da = residual_act_backward(a, b, dy, activation, p, seed, stream_id)                    # the gradient of a and of b
    y = residual_act(a, b, activation, p, seed, stream_id)                                  # differentiable
    lp = ctc_head_forward(x, weight, bias)                                                  # x fp16 [N][T][F] -> fp16 [N][T][classes]
    dx, dw, db = ctc_head_backward(x, weight, bias, dlp)
    lp = ctc_head(x, weight, bias)                                                          # differentiable

Activations are channel-minor: a convolution returns [N][Lout][Cout], or time-major [Lout][N][Cout] (the permute in front of the LSTM
stack, folded into the store). weight and bias are the fp32 master tensors in torch's layout ([Cout][Cin][K], [C][K]).

torch allocates and orders the streams; every number is computed by libbonito_hip.so. There is no PyTorch fallback: CPU tensors raise
NoTorchCompute, an unsupported shape or dtype raises ValueError before anything is launched.
"""
import math

import torch

from bonito_amd import _lib
from bonito_amd._train import (HalfLayer, HalfLayer2, act_name, devices as _devices, dtype_names as _dtype_names, half as _half,
                               master as _master, tensors as _tensors, workspace as _workspace)

__all__ = ["conv1d_forward", "conv1d_backward", "conv1d", "linear_forward", "linear_backward", "linear", "conv_out_len",
           "rmsnorm_residual_forward", "rmsnorm_residual_backward", "rmsnorm_residual",
           "gated_linear_forward", "gated_linear_backward", "gated_linear",
           "batchnorm_forward", "batchnorm_backward", "batchnorm",
           "depthwise_conv1d_forward", "depthwise_conv1d_backward", "depthwise_conv1d",
           "residual_act_forward", "residual_act_backward", "residual_act", "keep_threshold",
           "ctc_head_forward", "ctc_head_backward", "ctc_head"]

_INF = float("inf")


def conv_out_len(Lin, K, stride, padding):
    return (Lin + 2 * padding - K) // stride + 1


def _act(activation, allowed, what):
    name = act_name(activation)
    if name not in allowed:
        raise ValueError("%s: activation %r is not supported (one of %s)" % (what, name, ", ".join(str(a) for a in allowed)))
    return _lib.BH_ACT[name]


def _clamp(clamp, what):
    if clamp is None:
        return -_INF, _INF
    lo, hi = float(clamp[0]), float(clamp[1])
    if not lo <= hi:
        raise ValueError("%s: clamp range (%g, %g) is empty" % (what, lo, hi))
    return lo, hi


# ---- convolution ------------------------------------------------------------------------------------------------------------------------
def _conv_check(x, weight, bias, stride, padding, activation, clamp, what, dtypes=(torch.float16,), devices=True):
    named = [("x", x), ("weight", weight)] + ([("bias", bias)] if bias is not None else [])
    _tensors(named, what)
    if weight.dim() != 3:
        raise ValueError("%s: weight must be [Cout][Cin][K], got %s" % (what, tuple(weight.shape)))
    Cout, Cin, K = weight.shape
    if x.dtype not in dtypes:
        raise ValueError("%s: x must be %s, got %s" % (what, _dtype_names(dtypes), x.dtype))
    if not ((x.dim() == 3 and x.shape[2] == Cin) or (x.dim() == 2 and Cin == 1)) or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("%s: x must be [N][Lin][%d]%s, got %s" % (what, Cin, " or [N][Lin]" if Cin == 1 else "", tuple(x.shape)))
    _master(weight, (Cout, Cin, K), "weight", what)
    if bias is not None:
        _master(bias, (Cout,), "bias", what)
    N, Lin = int(x.shape[0]), int(x.shape[1])
    stride, padding = int(stride), int(padding)
    act = _act(activation, (None, "none", "swish", "tanh", "relu"), what)
    lo, hi = _clamp(clamp, what)
    if not (Cin == 1 or Cin % 8 == 0) or Cout % 4 != 0:
        raise ValueError("%s: Cin must be 1 or a multiple of 8 and Cout a multiple of 4 (Cin=%d Cout=%d)" % (what, Cin, Cout))
    if not (1 <= K <= 32 and 1 <= stride <= 8 and 0 <= padding < K and Lin + 2 * padding >= K):
        raise ValueError("%s: K <= 32, stride <= 8, padding < K and one whole window are needed (K=%d stride=%d padding=%d Lin=%d)"
                         % (what, K, stride, padding, Lin))
    if devices:
        _devices(named, what)
    return N, Lin, int(Cin), int(Cout), int(K), stride, padding, act, lo, hi


def _conv_strides(N, Lout, Cout, time_major):
    return (Cout, N * Cout) if time_major else (Lout * Cout, Cout)


def conv1d_forward(x, weight, bias=None, stride=1, padding=0, activation=None, clamp=None, time_major=False):
    """-> y fp16 [N][Lout][Cout], or [Lout][N][Cout] with time_major: the bytes bh_conv1d_first / bh_conv1d give on the rounded weights."""
    N, Lin, Cin, Cout, K, stride, padding, act, lo, hi = _conv_check(x, weight, bias, stride, padding, activation, clamp, "conv1d_forward")
    x, weight = x.contiguous(), weight.detach().contiguous()
    bias = None if bias is None else bias.detach().contiguous()
    lib = _lib.lib()
    nbytes = _workspace("bh_conv1d_train_workspace", "conv1d_forward", N=N, Lin=Lin, Cin=Cin, Cout=Cout, K=K, stride=stride, padding=padding)
    Lout = conv_out_len(Lin, K, stride, padding)
    os_n, os_t = _conv_strides(N, Lout, Cout, time_major)
    with torch.cuda.device(x.device):
        y = torch.empty((Lout, N, Cout) if time_major else (N, Lout, Cout), dtype=torch.float16, device=x.device)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _lib.check(lib.bh_conv1d_train_forward(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), N, Lin, Cin, Cout, K, stride, padding, act, lo, hi,
                                               os_n, os_t, _lib.ptr(y), _lib.ptr(ws), nbytes, _lib.stream_ptr(x.device)),
                   "bh_conv1d_train_forward")
    return y


def conv1d_backward(x, weight, bias, y, dy, stride=1, padding=0, activation=None, clamp=None, time_major=False, need_dx=True,
                    need_db=True):
    """-> (dx fp16 in the shape of x or None, dw fp32 [Cout][Cin][K], db fp32 [Cout] or None) from y and the upstream gradient dy (both
    fp16 in the layout conv1d_forward returned)."""
    what = "conv1d_backward"
    N, Lin, Cin, Cout, K, stride, padding, act, lo, hi = _conv_check(x, weight, bias, stride, padding, activation, clamp, what, devices=False)
    _tensors([("y", y), ("dy", dy)], what)
    Lout = conv_out_len(Lin, K, stride, padding)
    shape = (Lout, N, Cout) if time_major else (N, Lout, Cout)
    _half(y, shape, "y", what)
    _half(dy, shape, "dy", what)
    _devices([("x", x), ("weight", weight), ("y", y), ("dy", dy)] + ([("bias", bias)] if bias is not None else []), what)
    x, weight, y, dy = x.contiguous(), weight.detach().contiguous(), y.contiguous(), dy.contiguous()
    bias = None if bias is None else bias.detach().contiguous()
    lib = _lib.lib()
    nbytes = _workspace("bh_conv1d_train_workspace", what, N=N, Lin=Lin, Cin=Cin, Cout=Cout, K=K, stride=stride, padding=padding)
    os_n, os_t = _conv_strides(N, Lout, Cout, time_major)
    with torch.cuda.device(x.device):
        dx = torch.empty(x.shape, dtype=torch.float16, device=x.device) if need_dx else None
        dw = torch.empty((Cout, Cin, K), dtype=torch.float32, device=x.device)
        db = torch.empty(Cout, dtype=torch.float32, device=x.device) if need_db else None
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _lib.check(lib.bh_conv1d_train_backward(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(y), _lib.ptr(dy), N, Lin, Cin, Cout, K,
                                                stride, padding, act, lo, hi, os_n, os_t, _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db),
                                                _lib.ptr(ws), nbytes, _lib.stream_ptr(x.device)), "bh_conv1d_train_backward")
    return dx, dw, db


def conv1d(x, weight, bias=None, stride=1, padding=0, activation=None, clamp=None, time_major=False):
    """y fp16 of one convolution with its activation and clamp, differentiable with respect to x (fp16 or fp32; fp32 is cast to fp16 and
    its gradient comes back as fp32), weight and bias, each where requires_grad is set. An input channel count that is neither 1 nor a
    multiple of 8 (the 4 channels behind a first_conv_size = 4 layer) is served by zero channels: x and weight are padded to the next
    multiple of 8 and the gradients sliced back."""
    what = "conv1d"
    both = (torch.float16, torch.float32)
    _tensors([("x", x), ("weight", weight)], what)
    if weight.dim() == 3 and x.dim() == 3 and weight.shape[1] != 1 and weight.shape[1] % 8 != 0 and x.shape[2] == weight.shape[1]:
        if x.dtype not in both:
            raise ValueError("conv1d: x must be float16 or float32, got %s" % x.dtype)
        _master(weight, weight.shape, "weight", what)
        _devices([("x", x), ("weight", weight)], what)
        extra = -weight.shape[1] % 8
        x = torch.nn.functional.pad(x, (0, extra))
        weight = torch.nn.functional.pad(weight, (0, 0, 0, extra))
    _conv_check(x, weight, bias, stride, padding, activation, clamp, what, dtypes=both)
    args = (int(stride), int(padding), activation, clamp, bool(time_major))

    def forward(x16, weight, bias):
        y = conv1d_forward(x16, weight, bias, *args)
        return y, (x16, weight, bias, y)

    def backward(kept, dy, need):
        return conv1d_backward(*kept, dy, *args, need_dx=need[0], need_db=kept[2] is not None and need[2])

    return HalfLayer.apply(forward, backward, x, weight, bias)


# ---- linear -----------------------------------------------------------------------------------------------------------------------------
def _linear_check(x, weight, bias, activation, scale, clamp, what, dtypes=(torch.float16,), devices=True):
    named = [("x", x), ("weight", weight)] + ([("bias", bias)] if bias is not None else [])
    _tensors(named, what)
    if weight.dim() != 2:
        raise ValueError("%s: weight must be [C][K], got %s" % (what, tuple(weight.shape)))
    C, K = weight.shape
    if x.dtype not in dtypes:
        raise ValueError("%s: x must be %s, got %s" % (what, _dtype_names(dtypes), x.dtype))
    if x.dim() != 3 or x.shape[2] != K or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("%s: x must be [T][N][%d] with T, N >= 1, got %s" % (what, K, tuple(x.shape)))
    _master(weight, (C, K), "weight", what)
    if bias is not None:
        _master(bias, (C,), "bias", what)
    act = _act(activation, (None, "none", "tanh"), what)
    lo, hi = _clamp(clamp, what)
    scale = 1.0 if scale is None else float(scale)
    if scale == 0.0 or not math.isfinite(scale):
        raise ValueError("%s: scale must be finite and not 0, got %r" % (what, scale))
    if K % 8 != 0 or C % 8 != 0:
        raise ValueError("%s: K and C must be multiples of 8 (K=%d C=%d)" % (what, K, C))
    if devices:
        _devices(named, what)
    return int(x.shape[0]), int(x.shape[1]), int(K), int(C), act, scale, lo, hi


def linear_forward(x, weight, bias=None, activation=None, scale=None, clamp=None, batch_major_out=False):
    """-> Y fp16 [T][N][C], or [N][T][C] with batch_major_out (what Model.forward returns): the bytes of bh_linear on the rounded weights."""
    T, N, K, C, act, scale, lo, hi = _linear_check(x, weight, bias, activation, scale, clamp, "linear_forward")
    x, weight = x.contiguous(), weight.detach().contiguous()
    bias = None if bias is None else bias.detach().contiguous()
    lib = _lib.lib()
    nbytes = _workspace("bh_linear_train_workspace", "linear_forward", T=T, N=N, K=K, C=C)
    with torch.cuda.device(x.device):
        y = torch.empty((N, T, C) if batch_major_out else (T, N, C), dtype=torch.float16, device=x.device)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _lib.check(lib.bh_linear_train_forward(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), T, N, K, C, act, scale, lo, hi,
                                               int(bool(batch_major_out)), _lib.ptr(y), _lib.ptr(ws), nbytes, _lib.stream_ptr(x.device)),
                   "bh_linear_train_forward")
    return y


def linear_backward(x, weight, y, dy, activation=None, scale=None, clamp=None, batch_major_out=False, need_dx=True, need_db=True):
    """-> (dx fp16 [T][N][K] or None, dw fp32 [C][K], db fp32 [C] or None) from Y and the upstream gradient dy (fp16, in Y's layout)."""
    what = "linear_backward"
    T, N, K, C, act, scale, lo, hi = _linear_check(x, weight, None, activation, scale, clamp, what, devices=False)
    _tensors([("y", y), ("dy", dy)], what)
    shape = (N, T, C) if batch_major_out else (T, N, C)
    _half(y, shape, "y", what)
    _half(dy, shape, "dy", what)
    _devices([("x", x), ("weight", weight), ("y", y), ("dy", dy)], what)
    x, weight, y, dy = x.contiguous(), weight.detach().contiguous(), y.contiguous(), dy.contiguous()
    lib = _lib.lib()
    nbytes = _workspace("bh_linear_train_workspace", what, T=T, N=N, K=K, C=C)
    with torch.cuda.device(x.device):
        dx = torch.empty((T, N, K), dtype=torch.float16, device=x.device) if need_dx else None
        dw = torch.empty((C, K), dtype=torch.float32, device=x.device)
        db = torch.empty(C, dtype=torch.float32, device=x.device) if need_db else None
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _lib.check(lib.bh_linear_train_backward(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(y), _lib.ptr(dy), T, N, K, C, act, scale, lo, hi,
                                                int(bool(batch_major_out)), _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), nbytes,
                                                _lib.stream_ptr(x.device)), "bh_linear_train_backward")
    return dx, dw, db


def linear(x, weight, bias=None, activation=None, scale=None, clamp=None, batch_major_out=False):
    """Y fp16 of one linear layer or CRF head (activation none or tanh, scale, clamp), differentiable with respect to x (fp16 or fp32;
    fp32 is cast to fp16 and its gradient comes back as fp32), weight and bias, each where requires_grad is set."""
    _linear_check(x, weight, bias, activation, scale, clamp, "linear", dtypes=(torch.float16, torch.float32))
    args = (activation, scale, clamp, bool(batch_major_out))

    def forward(x16, weight, bias):
        y = linear_forward(x16, weight, bias, *args)
        return y, (x16, weight, y)

    def backward(kept, dy, need):
        return linear_backward(*kept, dy, *args, need_dx=need[0], need_db=bias is not None and need[2])

    return HalfLayer.apply(forward, backward, x, weight, bias)


# ---- DeepNorm residual RMSNorm --------------------------------------------------------------------------------------------------------------
_BOTH = (torch.float16, torch.float32)


def _norm_check(a, x, weight, alpha, eps, what, dtypes=(torch.float16,), devices=True):
    named = [("a", a), ("x", x), ("weight", weight)]
    _tensors(named, what)
    for name, t in named[:2]:
        if t.dtype not in dtypes:
            raise ValueError("%s: %s must be %s, got %s" % (what, name, _dtype_names(dtypes), t.dtype))
    if a.dim() < 2 or a.numel() == 0 or a.shape != x.shape:
        raise ValueError("%s: a and x must be [...][D] of one shape, got %s and %s" % (what, tuple(a.shape), tuple(x.shape)))
    D = int(a.shape[-1])
    _master(weight, (D,), "weight", what)
    if isinstance(alpha, torch.Tensor) and alpha.numel() != 1:
        raise ValueError("%s: alpha must be one number, got a tensor %s" % (what, tuple(alpha.shape)))
    alpha, eps = float(alpha), float(eps)
    if not math.isfinite(alpha) or not math.isfinite(eps) or eps < 0.0:
        raise ValueError("%s: alpha must be finite and eps finite and >= 0, got %r and %r" % (what, alpha, eps))
    if D % 8 != 0 or not 8 <= D <= 1024:
        raise ValueError("%s: D must be a multiple of 8 in 8..1024, got %d" % (what, D))
    if devices:
        _devices(named, what)
    return a.numel() // D, D, alpha, eps


def rmsnorm_residual_forward(a, x, weight, alpha, eps=1e-5):
    """-> out fp16 in the shape of a: rmsnorm(a + alpha x) weight, the bytes of bh_rmsnorm_residual (a, x fp16 [...][D], weight fp32 [D])."""
    M, D, alpha, eps = _norm_check(a, x, weight, alpha, eps, "rmsnorm_residual_forward")
    a, x, weight = a.contiguous(), x.contiguous(), weight.detach().contiguous()
    with torch.cuda.device(a.device):
        out = torch.empty_like(a)
        _lib.check(_lib.lib().bh_rmsnorm_residual(_lib.ptr(a), _lib.ptr(x), _lib.ptr(weight), _lib.ptr(out), M, D, alpha, eps,
                                                  _lib.stream_ptr(a.device)), "bh_rmsnorm_residual")
    return out


def rmsnorm_residual_backward(a, x, weight, dy, alpha, eps=1e-5, need_da=True, need_dx=True):
    """-> (da fp16 or None, dx fp16 or None, dw fp32 [D]) from the upstream gradient dy (fp16, in the shape of a); nothing of the forward
    is needed: z and r are recomputed from a and x."""
    what = "rmsnorm_residual_backward"
    M, D, alpha, eps = _norm_check(a, x, weight, alpha, eps, what, devices=False)
    _tensors([("dy", dy)], what)
    _half(dy, a.shape, "dy", what)
    _devices([("a", a), ("x", x), ("weight", weight), ("dy", dy)], what)
    a, x, weight, dy = a.contiguous(), x.contiguous(), weight.detach().contiguous(), dy.contiguous()
    lib = _lib.lib()
    nbytes = _workspace("bh_rmsnorm_train_workspace", what, M=M, D=D)
    with torch.cuda.device(a.device):
        da = torch.empty_like(a) if need_da else None
        dx = torch.empty_like(a) if need_dx else None
        dw = torch.empty(D, dtype=torch.float32, device=a.device)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
        _lib.check(lib.bh_rmsnorm_train_backward(_lib.ptr(a), _lib.ptr(x), _lib.ptr(weight), _lib.ptr(dy), M, D, alpha, eps, _lib.ptr(da),
                                                 _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(ws), nbytes, _lib.stream_ptr(a.device)),
                   "bh_rmsnorm_train_backward")
    return da, dx, dw


def rmsnorm_residual(a, x, weight, alpha, eps=1e-5):
    """out fp16 = rmsnorm(a + alpha x) weight, differentiable with respect to a, x (each fp16 or fp32; fp32 is cast to fp16 and its
    gradient comes back as fp32) and weight, each where requires_grad is set. alpha (a number or a one-element tensor) gets no gradient."""
    _, _, alpha, eps = _norm_check(a, x, weight, alpha, eps, "rmsnorm_residual", dtypes=_BOTH)

    def forward(a16, x16, weight):
        return rmsnorm_residual_forward(a16, x16, weight, alpha, eps), (a16, x16, weight)

    def backward(kept, dy, need):
        return rmsnorm_residual_backward(*kept, dy.contiguous(), alpha, eps, need_da=need[0], need_dx=need[1])

    return HalfLayer2.apply(forward, backward, a, x, weight)


# ---- gated input layer of the MLP (fc1 + SwiGLU) ----------------------------------------------------------------------------------------------
def _gated_check(x, weight, what, dtypes=(torch.float16,), devices=True):
    named = [("x", x), ("weight", weight)]
    _tensors(named, what)
    if weight.dim() != 2 or weight.shape[0] % 2 != 0:
        raise ValueError("%s: weight must be [2F][D] (y rows, then gate rows), got %s" % (what, tuple(weight.shape)))
    F, D = int(weight.shape[0]) // 2, int(weight.shape[1])
    if x.dtype not in dtypes:
        raise ValueError("%s: x must be %s, got %s" % (what, _dtype_names(dtypes), x.dtype))
    if x.dim() < 2 or x.shape[-1] != D or x.numel() == 0:
        raise ValueError("%s: x must be [...][%d], got %s" % (what, D, tuple(x.shape)))
    _master(weight, (2 * F, D), "weight", what)
    if D % 8 != 0 or F % 8 != 0 or F < 8:
        raise ValueError("%s: D and F must be multiples of 8 (D=%d F=%d)" % (what, D, F))
    if devices:
        _devices(named, what)
    return x.numel() // D, D, F


def gated_linear_forward(x, weight):
    """-> h fp16 [...][F] = y gate sigmoid(gate), [y | gate] = x weight^T (x fp16 [...][D], weight fp32 [2F][D]): the bytes of bh_linear with
    gated = 1 on the rounded, row-interleaved weights, which is the engine's fc1."""
    what = "gated_linear_forward"
    M, D, F = _gated_check(x, weight, what)
    x, weight = x.contiguous(), weight.detach().contiguous()
    nbytes = _workspace("bh_gated_linear_train_workspace", what, M=M, D=D, F=F)
    with torch.cuda.device(x.device):
        h = torch.empty(tuple(x.shape[:-1]) + (F,), dtype=torch.float16, device=x.device)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _lib.check(_lib.lib().bh_gated_linear_train_forward(_lib.ptr(x), _lib.ptr(weight), M, D, F, _lib.ptr(h), _lib.ptr(ws), nbytes,
                                                            _lib.stream_ptr(x.device)), "bh_gated_linear_train_forward")
    return h


def gated_linear_backward(x, weight, dh, need_dx=True):
    """-> (dx fp16 in the shape of x or None, dw fp32 [2F][D] in torch's row order) from the upstream gradient dh (fp16 [...][F]); y and gate
    are recomputed."""
    what = "gated_linear_backward"
    M, D, F = _gated_check(x, weight, what, devices=False)
    _tensors([("dh", dh)], what)
    _half(dh, tuple(x.shape[:-1]) + (F,), "dh", what)
    _devices([("x", x), ("weight", weight), ("dh", dh)], what)
    x, weight, dh = x.contiguous(), weight.detach().contiguous(), dh.contiguous()
    nbytes = _workspace("bh_gated_linear_train_workspace", what, M=M, D=D, F=F)
    with torch.cuda.device(x.device):
        dx = torch.empty_like(x) if need_dx else None
        dw = torch.empty((2 * F, D), dtype=torch.float32, device=x.device)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _lib.check(_lib.lib().bh_gated_linear_train_backward(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(dh), M, D, F, _lib.ptr(dx), _lib.ptr(dw),
                                                             _lib.ptr(ws), nbytes, _lib.stream_ptr(x.device)), "bh_gated_linear_train_backward")
    return dx, dw


def gated_linear(x, weight):
    """h fp16 [...][F] of the gated input layer, differentiable with respect to x (fp16 or fp32; fp32 is cast to fp16 and its gradient
    comes back as fp32) and weight, each where requires_grad is set."""
    _gated_check(x, weight, "gated_linear", dtypes=_BOTH)

    def forward(x16, weight):
        x16 = x16.contiguous()
        return gated_linear_forward(x16, weight), (x16, weight)

    def backward(kept, dh, need):
        return gated_linear_backward(*kept, dh.contiguous(), need_dx=need[0])

    return HalfLayer.apply(forward, backward, x, weight)


# ---- batch-statistics BatchNorm behind a convolution ------------------------------------------------------------------------------------------
def _bn_check(z, weight, bias, activation, clamp, channels, what, dtypes=(torch.float16,), devices=True):
    named = [("z", z)] + [(n, t) for n, t in (("weight", weight), ("bias", bias)) if t is not None]
    _tensors(named, what)
    if z.dtype not in dtypes:
        raise ValueError("%s: z must be %s, got %s" % (what, _dtype_names(dtypes), z.dtype))
    if z.dim() != 3 or z.numel() == 0:
        raise ValueError("%s: z must be [N][L][C], got %s" % (what, tuple(z.shape)))
    N, L, C = (int(v) for v in z.shape)
    if (weight is None) != (bias is None):
        raise ValueError("%s: weight and bias come together or not at all (affine)" % what)
    if weight is not None:
        _master(weight, (C,), "weight", what)
        _master(bias, (C,), "bias", what)
    act = _act(activation, (None, "none", "swish", "tanh", "relu"), what)
    lo, hi = _clamp(clamp, what)
    if C % 8 != 0 or C > 2048:
        raise ValueError("%s: C must be a multiple of 8 up to 2048, got %d" % (what, C))
    Cp = C if channels is None else int(channels)
    if not 1 <= Cp <= C:
        raise ValueError("%s: channels must be in 1..%d, got %d" % (what, C, Cp))
    if N * L < 2:
        raise ValueError("%s: more than one value per channel is needed, got z %s" % (what, tuple(z.shape)))
    if devices:
        _devices(named, what)
    return N, L, C, Cp, act, lo, hi


def _bn_strides(N, L, C, time_major):
    return (C, N * C) if time_major else (L * C, C)


def batchnorm_forward(z, weight, bias, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, activation=None, clamp=None,
                      time_major=False, channels=None):
    """-> (y fp16 [N][L][C], or [L][N][C] with time_major; mean fp32 [C]; rstd fp32 [C]) of torch.nn.BatchNorm1d in training mode on
    z fp16 [N][L][C] (channel-minor), with the activation and the clamp: y = clamp(act(weight (z - mean) rstd + bias)). weight and bias
    are fp32 [C], or both None (affine=False). running_mean / running_var (fp32 [channels], or both None) are UPDATED IN PLACE with
    `momentum` and the unbiased variance, as torch does. channels < C: the channels behind are zero padding - y is 0 there, mean and rstd
    stay 0, and weight and bias are not read there."""
    what = "batchnorm_forward"
    N, L, C, Cp, act, lo, hi = _bn_check(z, weight, bias, activation, clamp, channels, what, devices=False)
    if (running_mean is None) != (running_var is None):
        raise ValueError("%s: running_mean and running_var come together or not at all (track_running_stats)" % what)
    named = [("z", z)] + [(n, t) for n, t in (("weight", weight), ("bias", bias), ("running_mean", running_mean),
                                              ("running_var", running_var)) if t is not None]
    _tensors(named, what)
    if running_mean is not None:
        for name, t in named[-2:]:
            _master(t, (Cp,), name, what)
            if not t.is_contiguous():
                raise ValueError("%s: %s must be contiguous (it is updated in place)" % (what, name))
        if momentum is None:
            raise ValueError("%s: momentum=None (the cumulative average) is not served" % what)
    momentum, eps = 0.0 if momentum is None else float(momentum), float(eps)
    if not 0.0 <= momentum <= 1.0:
        raise ValueError("%s: momentum must be in 0..1, got %r" % (what, momentum))
    if not (math.isfinite(eps) and eps > 0.0):
        raise ValueError("%s: eps must be finite and > 0, got %r" % (what, eps))
    _devices(named, what)
    z = z.contiguous()
    weight, bias = (None, None) if weight is None else (weight.detach().contiguous(), bias.detach().contiguous())
    nbytes = _workspace("bh_batchnorm_train_workspace", what, N=N, L=L, C=C)
    os_n, os_t = _bn_strides(N, L, C, time_major)
    with torch.cuda.device(z.device):
        y = torch.empty((L, N, C) if time_major else (N, L, C), dtype=torch.float16, device=z.device)
        mean = torch.zeros(C, dtype=torch.float32, device=z.device)
        rstd = torch.zeros(C, dtype=torch.float32, device=z.device)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=z.device)
        _lib.check(_lib.lib().bh_batchnorm_train_forward(_lib.ptr(z), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(running_mean),
                                                         _lib.ptr(running_var), N, L, C, Cp, eps, momentum, act, lo, hi, os_n, os_t, _lib.ptr(y),
                                                         _lib.ptr(mean), _lib.ptr(rstd), _lib.ptr(ws), nbytes, _lib.stream_ptr(z.device)),
                   "bh_batchnorm_train_forward")
    return y, mean, rstd


def batchnorm_backward(z, weight, bias, mean, rstd, y, dy, activation=None, clamp=None, time_major=False, channels=None, need_dw=True,
                       need_db=True):
    """-> (dz fp16 [N][L][C], dw fp32 [C] or None, db fp32 [C] or None) from what batchnorm_forward returned and the upstream gradient
    dy (fp16, in y's layout). Padded channels get zeros."""
    what = "batchnorm_backward"
    N, L, C, Cp, act, lo, hi = _bn_check(z, weight, bias, activation, clamp, channels, what, devices=False)
    _tensors([("mean", mean), ("rstd", rstd), ("y", y), ("dy", dy)], what)
    _master(mean, (C,), "mean", what)
    _master(rstd, (C,), "rstd", what)
    shape = (L, N, C) if time_major else (N, L, C)
    _half(y, shape, "y", what)
    _half(dy, shape, "dy", what)
    _devices([("z", z), ("mean", mean), ("rstd", rstd), ("y", y), ("dy", dy)]
             + ([("weight", weight), ("bias", bias)] if weight is not None else []), what)
    z, mean, rstd, y, dy = z.contiguous(), mean.contiguous(), rstd.contiguous(), y.contiguous(), dy.contiguous()
    weight, bias = (None, None) if weight is None else (weight.detach().contiguous(), bias.detach().contiguous())
    nbytes = _workspace("bh_batchnorm_train_workspace", what, N=N, L=L, C=C)
    os_n, os_t = _bn_strides(N, L, C, time_major)
    with torch.cuda.device(z.device):
        dz = torch.empty((N, L, C), dtype=torch.float16, device=z.device)
        dw = torch.zeros(C, dtype=torch.float32, device=z.device) if need_dw else None
        db = torch.zeros(C, dtype=torch.float32, device=z.device) if need_db else None
        ws = torch.empty(nbytes, dtype=torch.uint8, device=z.device)
        _lib.check(_lib.lib().bh_batchnorm_train_backward(_lib.ptr(z), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(mean), _lib.ptr(rstd),
                                                          _lib.ptr(y), _lib.ptr(dy), N, L, C, Cp, act, lo, hi, os_n, os_t, _lib.ptr(dz),
                                                          _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), nbytes, _lib.stream_ptr(z.device)),
                   "bh_batchnorm_train_backward")
    return dz, dw, db


def batchnorm(z, weight, bias, running_mean=None, running_var=None, momentum=0.1, eps=1e-5, activation=None, clamp=None, time_major=False,
              channels=None):
    """y fp16 of batch-statistics BatchNorm with its activation and clamp, differentiable with respect to z (fp16 or fp32; fp32 is cast
    to fp16 and its gradient comes back as fp32), weight and bias, each where requires_grad is set. The forward - and only the forward -
    updates running_mean / running_var in place, under torch.no_grad() too, as torch.nn.BatchNorm1d in training mode does."""
    _bn_check(z, weight, bias, activation, clamp, channels, "batchnorm", dtypes=_BOTH)
    args = (activation, clamp, bool(time_major), channels)

    def forward(z16, weight, bias):
        z16 = z16.contiguous()
        y, mean, rstd = batchnorm_forward(z16, weight, bias, running_mean, running_var, momentum, eps, *args)
        return y, (z16, weight, bias, mean, rstd, y)

    def backward(kept, dy, need):
        affine = kept[1] is not None
        return batchnorm_backward(*kept, dy.contiguous(), *args, need_dw=affine and need[1], need_db=affine and need[2])

    return HalfLayer.apply(forward, backward, z, weight, bias)


# ---- depthwise convolution (QuartzNet's TCSConv1d.depthwise) --------------------------------------------------------------------------------
def _dw_check(x, weight, padding, what, dtypes=(torch.float16,), devices=True):
    named = [("x", x), ("weight", weight)]
    _tensors(named, what)
    if weight.dim() != 3 or weight.shape[1] != 1:
        raise ValueError("%s: weight must be [C][1][K] (groups = C), got %s" % (what, tuple(weight.shape)))
    C, K = int(weight.shape[0]), int(weight.shape[2])
    if x.dtype not in dtypes:
        raise ValueError("%s: x must be %s, got %s" % (what, _dtype_names(dtypes), x.dtype))
    if x.dim() != 3 or x.shape[2] != C or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("%s: x must be [N][L][%d], got %s" % (what, C, tuple(x.shape)))
    _master(weight, (C, 1, K), "weight", what)
    N, L, padding = int(x.shape[0]), int(x.shape[1]), int(padding)
    if C % 8 != 0:
        raise ValueError("%s: C must be a multiple of 8, got %d" % (what, C))
    if not (1 <= K <= 127 and 0 <= padding < K and L + 2 * padding >= K):
        raise ValueError("%s: K <= 127, padding < K and one whole window are needed (K=%d padding=%d L=%d)" % (what, K, padding, L))
    if devices:
        _devices(named, what)
    return N, L, C, K, padding


def depthwise_conv1d_forward(x, weight, padding=0):
    """-> y fp16 [N][Lout][C]: the bytes of bh_dwconv1d (stride 1) on the fp32 weights, used unrounded."""
    N, L, C, K, padding = _dw_check(x, weight, padding, "depthwise_conv1d_forward")
    x, weight = x.contiguous(), weight.detach().contiguous()
    with torch.cuda.device(x.device):
        y = torch.empty((N, conv_out_len(L, K, 1, padding), C), dtype=torch.float16, device=x.device)
        _lib.check(_lib.lib().bh_dwconv1d(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(y), N, L, C, K, 1, padding, _lib.stream_ptr(x.device)),
                   "bh_dwconv1d")
    return y


def depthwise_conv1d_backward(x, weight, dy, padding=0, need_dx=True, need_dw=True):
    """-> (dx fp16 in the shape of x or None, dw fp32 [C][1][K] or None) from the upstream gradient dy (fp16 [N][Lout][C])."""
    what = "depthwise_conv1d_backward"
    N, L, C, K, padding = _dw_check(x, weight, padding, what, devices=False)
    _tensors([("dy", dy)], what)
    _half(dy, (N, conv_out_len(L, K, 1, padding), C), "dy", what)
    _devices([("x", x), ("weight", weight), ("dy", dy)], what)
    x, weight, dy = x.contiguous(), weight.detach().contiguous(), dy.contiguous()
    lib = _lib.lib()
    nbytes = _workspace("bh_dwconv1d_train_workspace", what, N=N, L=L, C=C, K=K, padding=padding)
    with torch.cuda.device(x.device):
        dx = torch.empty_like(x) if need_dx else None
        dw = torch.empty((C, 1, K), dtype=torch.float32, device=x.device) if need_dw else None
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _lib.check(lib.bh_dwconv1d_train_backward(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(dy), N, L, C, K, padding, _lib.ptr(dx), _lib.ptr(dw),
                                                  _lib.ptr(ws), nbytes, _lib.stream_ptr(x.device)), "bh_dwconv1d_train_backward")
    return dx, dw


def depthwise_conv1d(x, weight, padding=0):
    """y fp16 [N][Lout][C] of a depthwise convolution (stride 1, dilation 1, no bias), differentiable with respect to x (fp16 or fp32;
    fp32 is cast to fp16 and its gradient comes back as fp32) and weight, each where requires_grad is set."""
    _dw_check(x, weight, padding, "depthwise_conv1d", dtypes=_BOTH)
    padding = int(padding)

    def forward(x16, weight):
        x16 = x16.contiguous()
        return depthwise_conv1d_forward(x16, weight, padding), (x16, weight)

    def backward(kept, dy, need):
        return depthwise_conv1d_backward(*kept, dy.contiguous(), padding, need_dx=need[0], need_dw=need[1])

    return HalfLayer.apply(forward, backward, x, weight)


# ---- residual add + activation + dropout -----------------------------------------------------------------------------------------------------
def keep_threshold(p):
    """-> (p_threshold, inv_keep) of a dropout probability: floor(p 2^32) in double and 1 / (1 - p); an element is kept iff the top 32
    bits of its counter-based hash reach p_threshold (include/bonito_hip.h)."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout probability must be in 0 <= p < 1, got %r" % p)
    return int(math.floor(p * 4294967296.0)), 1.0 / (1.0 - p)


def _res_check(a, b, activation, p, seed, stream_id, what, dtypes=(torch.float16,), devices=True):
    named = [("a", a)] + ([("b", b)] if b is not None else [])
    _tensors(named, what)
    for name, t in named:
        if t.dtype not in dtypes:
            raise ValueError("%s: %s must be %s, got %s" % (what, name, _dtype_names(dtypes), t.dtype))
    if a.dim() < 2 or a.numel() == 0 or (b is not None and b.shape != a.shape):
        raise ValueError("%s: a and b must be [...][C] of one shape, got %s%s" % (what, tuple(a.shape), "" if b is None else " and %s" % (tuple(b.shape),)))
    C = int(a.shape[-1])
    act = _act(activation, (None, "none", "swish", "tanh", "relu"), what)
    try:
        threshold, inv_keep = keep_threshold(p)
    except ValueError as exc:
        raise ValueError("%s: %s" % (what, exc)) from None
    seed, stream_id = int(seed), int(stream_id)
    if not (0 <= seed < 1 << 64 and 0 <= stream_id < 1 << 64):
        raise ValueError("%s: seed and stream_id must be in 0..2^64-1, got %d and %d" % (what, seed, stream_id))
    if C % 8 != 0:
        raise ValueError("%s: C must be a multiple of 8, got %d" % (what, C))
    if devices:
        _devices(named, what)
    return a.numel() // C, C, act, threshold, inv_keep, seed, stream_id


def residual_act_forward(a, b, activation=None, p=0.0, seed=0, stream_id=0):
    """-> y fp16 in the shape of a: dropout(act(a + b)), b may be None. The mask is a function of (seed, stream_id, element index)."""
    M, C, act, threshold, inv_keep, seed, stream_id = _res_check(a, b, activation, p, seed, stream_id, "residual_act_forward")
    a, b = a.contiguous(), None if b is None else b.contiguous()
    with torch.cuda.device(a.device):
        y = torch.empty_like(a)
        _lib.check(_lib.lib().bh_residual_act_train_forward(_lib.ptr(a), _lib.ptr(b), M, C, act, threshold, inv_keep, seed, stream_id,
                                                            _lib.ptr(y), _lib.stream_ptr(a.device)), "bh_residual_act_train_forward")
    return y


def residual_act_backward(a, b, dy, activation=None, p=0.0, seed=0, stream_id=0):
    """-> da fp16 in the shape of a, which is the gradient of b too, from the upstream gradient dy; a + b and the mask are recomputed."""
    what = "residual_act_backward"
    M, C, act, threshold, inv_keep, seed, stream_id = _res_check(a, b, activation, p, seed, stream_id, what, devices=False)
    _tensors([("dy", dy)], what)
    _half(dy, a.shape, "dy", what)
    _devices([("a", a), ("dy", dy)] + ([("b", b)] if b is not None else []), what)
    a, b, dy = a.contiguous(), None if b is None else b.contiguous(), dy.contiguous()
    with torch.cuda.device(a.device):
        da = torch.empty_like(a)
        _lib.check(_lib.lib().bh_residual_act_train_backward(_lib.ptr(a), _lib.ptr(b), _lib.ptr(dy), M, C, act, threshold, inv_keep, seed,
                                                             stream_id, _lib.ptr(da), _lib.stream_ptr(a.device)),
                   "bh_residual_act_train_backward")
    return da


def residual_act(a, b=None, activation=None, p=0.0, seed=0, stream_id=0):
    """y fp16 = dropout_p(act(a + b)) (b may be None), differentiable with respect to a and b (each fp16 or fp32; fp32 is cast to fp16 and
    its gradient comes back as fp32). Nothing of the mask is stored: forward and backward compute it from (seed, stream_id, index)."""
    _res_check(a, b, activation, p, seed, stream_id, "residual_act", dtypes=_BOTH)
    args = (activation, float(p), int(seed), int(stream_id))
    if b is None:
        def forward(a16):
            a16 = a16.contiguous()
            return residual_act_forward(a16, None, *args), (a16,)

        def backward(kept, dy, need):
            return (residual_act_backward(kept[0], None, dy.contiguous(), *args),)

        return HalfLayer.apply(forward, backward, a)

    def forward2(a16, b16):
        a16, b16 = a16.contiguous(), b16.contiguous()
        return residual_act_forward(a16, b16, *args), (a16, b16)

    def backward2(kept, dy, need):
        da = residual_act_backward(*kept, dy.contiguous(), *args)
        return da, da

    return HalfLayer2.apply(forward2, backward2, a, b)


# ---- the 1x1 decoder with its log-softmax (QuartzNet's Decoder) ---------------------------------------------------------------------------------
def _head_check(x, weight, bias, what, dtypes=(torch.float16,), devices=True):
    named = [("x", x), ("weight", weight), ("bias", bias)]
    _tensors(named, what)
    if weight.dim() != 3 or weight.shape[2] != 1:
        raise ValueError("%s: weight must be [classes][F][1], got %s" % (what, tuple(weight.shape)))
    classes, F = int(weight.shape[0]), int(weight.shape[1])
    if x.dtype not in dtypes:
        raise ValueError("%s: x must be %s, got %s" % (what, _dtype_names(dtypes), x.dtype))
    if x.dim() != 3 or x.shape[2] != F or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("%s: x must be [N][T][%d], got %s" % (what, F, tuple(x.shape)))
    _master(weight, (classes, F, 1), "weight", what)
    _master(bias, (classes,), "bias", what)
    if not 1 <= classes <= 8 or F % 8 != 0 or classes * F * 4 > 65536:
        raise ValueError("%s: classes <= 8, F %% 8 == 0 and classes F fp32 weights within 64 KiB are needed (classes=%d F=%d)"
                         % (what, classes, F))
    if devices:
        _devices(named, what)
    return int(x.shape[0]), int(x.shape[1]), F, classes


def ctc_head_forward(x, weight, bias):
    """-> log-probabilities fp16 [N][T][classes]: the bytes of bh_ctc_head on the fp32 weights."""
    N, T, F, classes = _head_check(x, weight, bias, "ctc_head_forward")
    x, weight, bias = x.contiguous(), weight.detach().contiguous(), bias.detach().contiguous()
    with torch.cuda.device(x.device):
        lp = torch.empty((N, T, classes), dtype=torch.float16, device=x.device)
        _lib.check(_lib.lib().bh_ctc_head(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(lp), N * T, F, classes,
                                          _lib.stream_ptr(x.device)), "bh_ctc_head")
    return lp


def ctc_head_backward(x, weight, bias, dlp, need_dx=True, need_dw=True, need_db=True):
    """-> (dx fp16 [N][T][F] or None, dw fp32 [classes][F][1] or None, db fp32 [classes] or None) from dlp, the gradient of the
    log-probabilities (fp16 [N][T][classes]); the logits and their softmax are recomputed in fp32."""
    what = "ctc_head_backward"
    N, T, F, classes = _head_check(x, weight, bias, what, devices=False)
    _tensors([("dlp", dlp)], what)
    _half(dlp, (N, T, classes), "dlp", what)
    _devices([("x", x), ("weight", weight), ("bias", bias), ("dlp", dlp)], what)
    x, weight, bias, dlp = x.contiguous(), weight.detach().contiguous(), bias.detach().contiguous(), dlp.contiguous()
    lib = _lib.lib()
    nbytes = _workspace("bh_ctc_head_train_workspace", what, M=N * T, F=F, classes=classes)
    with torch.cuda.device(x.device):
        dx = torch.empty_like(x) if need_dx else None
        dw = torch.empty((classes, F, 1), dtype=torch.float32, device=x.device) if need_dw else None
        db = torch.empty(classes, dtype=torch.float32, device=x.device) if need_db else None
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _lib.check(lib.bh_ctc_head_train_backward(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(dlp), N * T, F, classes, _lib.ptr(dx),
                                                  _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), nbytes, _lib.stream_ptr(x.device)),
                   "bh_ctc_head_train_backward")
    return dx, dw, db


def ctc_head(x, weight, bias):
    """Log-probabilities fp16 [N][T][classes] of the 1x1 decoder, differentiable with respect to x (fp16 or fp32; fp32 is cast to fp16 and
    its gradient comes back as fp32), weight and bias, each where requires_grad is set."""
    _head_check(x, weight, bias, "ctc_head", dtypes=_BOTH)

    def forward(x16, weight, bias):
        x16 = x16.contiguous()
        return ctc_head_forward(x16, weight, bias), (x16, weight, bias)

    def backward(kept, dlp, need):
        return ctc_head_backward(*kept, dlp.contiguous(), need_dx=need[0], need_dw=need[1], need_db=need[2])

    return HalfLayer.apply(forward, backward, x, weight, bias)

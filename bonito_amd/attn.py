"""
The attention layer of a transformer model for training on the device: rotary embedding + sliding-window attention on packed qkv, the
forward that keeps what the backward needs, the backward, and their autograd (csrc/attention_train.hip; the arithmetic is stated in
include/bonito_hip.h under bh_attention_train_forward).

    out, saved = attention_forward(qkv, window)            # qkv fp16 [N][T][3][H][64] (or [N][T][3*H*64]); out fp16 [N][T][H*64]
    dqkv       = attention_backward(qkv, out, saved, dout, window)
    out        = attention(qkv, window)                    # differentiable with respect to qkv (fp16 or fp32)
    y          = mha_module(layer, x)                      # a transformer.model.MultiHeadAttention container, x [N][T][D]
    y          = encoder_layer(layer, x)                   # a transformer.model.TransformerEncoderLayer container: attention, the two
                                                           # DeepNorm residual RMSNorms and the gated MLP (bonito_amd.train_ops)

window = (left, right): key j is visible to query i of the same chunk iff i - left <= j <= i + right. torch allocates and orders the
streams; every number is computed by libbonito_hip.so. There is no PyTorch fallback: CPU tensors raise NoTorchCompute, an unsupported
shape, dtype or window raises ValueError before anything is launched.
"""
import numpy as np
import torch

from bonito_amd import _lib
from bonito_amd._train import HalfLayer, devices, dtype_names, half_dev, tensors, workspace

__all__ = ["attention_forward", "attention_backward", "attention", "mha_module", "encoder_layer", "encoder_layer_check", "supported_window",
           "HEAD_DIM"]

HEAD_DIM = 64
_tables = {}      # (device, T) -> the device copy of bh_rotary_table(T, 64)


def supported_window(window):
    """A finite window the kernels serve: left, right >= 0 and at most 26 key tiles of 16 per wave.
    The 26 must equal BH_ATTN_MAX_TILES of csrc/kernels.h (bh_k_attention_serves)."""
    try:
        wl, wr = (int(w) for w in window)
    except (TypeError, ValueError):
        return False
    return wl >= 0 and wr >= 0 and (16 + wl + wr + 15) // 16 <= 26


def _window(window, what):
    try:
        wl, wr = window
        wl, wr = int(wl), int(wr)
    except (TypeError, ValueError):
        raise ValueError("%s: window must be (left, right), got %r" % (what, window))
    if wl < 0 or wr < 0:
        raise ValueError("%s: a finite window (left, right) with left, right >= 0 is required, got (%d, %d)" % (what, wl, wr))
    if not supported_window((wl, wr)):
        raise ValueError("%s: window (%d, %d) is too wide for the kernels ((16 + left + right + 15) // 16 <= 26)" % (what, wl, wr))
    return wl, wr


def _shape(qkv, what):
    """-> (N, T, H) of a packed qkv [N][T][3][H][64] or [N][T][3*H*64]."""
    if qkv.dim() == 5:
        N, T, three, H, d = qkv.shape
        if d != HEAD_DIM:
            raise ValueError("%s: only head_dim %d is served, got %d" % (what, HEAD_DIM, d))
        if three != 3:
            raise ValueError("%s: qkv must be [N][T][3][H][%d], got %s" % (what, HEAD_DIM, tuple(qkv.shape)))
    elif qkv.dim() == 3:
        N, T, W = qkv.shape
        if W % (3 * HEAD_DIM) != 0:
            raise ValueError("%s: qkv must be [N][T][3*H*%d] (head_dim %d), got %s" % (what, HEAD_DIM, HEAD_DIM, tuple(qkv.shape)))
        H = W // (3 * HEAD_DIM)
    else:
        raise ValueError("%s: qkv must be [N][T][3][H][%d] or [N][T][3*H*%d], got %s" % (what, HEAD_DIM, HEAD_DIM, tuple(qkv.shape)))
    if N < 1 or T < 1 or H < 1:
        raise ValueError("%s: N, T and H must be at least 1, got %s" % (what, tuple(qkv.shape)))
    return int(N), int(T), int(H)


def _check(qkv, window, what, dtypes=(torch.float16,)):
    tensors([("qkv", qkv)], what)
    if qkv.dtype not in dtypes:
        raise ValueError("%s: qkv must be %s, got %s" % (what, dtype_names(dtypes), qkv.dtype))
    N, T, H = _shape(qkv, what)
    wl, wr = _window(window, what)
    devices([("qkv", qkv)], what)
    return N, T, H, wl, wr


def _table(device, T):
    key = (device, T)
    if key not in _tables:
        tab = np.empty((T, HEAD_DIM // 2, 2), np.float32)
        _lib.check(_lib.lib().bh_rotary_table(T, HEAD_DIM, tab.ctypes.data), "bh_rotary_table")
        _tables[key] = torch.from_numpy(tab).to(device)
    return _tables[key]


def attention_forward(qkv, window):
    """-> (out fp16 [N][T][H*64] with the bytes of bh_attention, saved): `saved` is the opaque byte buffer attention_backward needs."""
    N, T, H, wl, wr = _check(qkv, window, "attention_forward")
    qkv = qkv.contiguous()
    lib = _lib.lib()
    nbytes = workspace("bh_attention_train_saved_bytes", "attention_forward", N=N, T=T, H=H)
    with torch.cuda.device(qkv.device):
        tab = _table(qkv.device, T)
        out = torch.empty((N, T, H * HEAD_DIM), dtype=torch.float16, device=qkv.device)
        saved = torch.empty(nbytes, dtype=torch.uint8, device=qkv.device)
        _lib.check(lib.bh_attention_train_forward(_lib.ptr(qkv), _lib.ptr(tab), N, T, H, HEAD_DIM, wl, wr, _lib.ptr(out), _lib.ptr(saved),
                                                  nbytes, _lib.stream_ptr(qkv.device)), "bh_attention_train_forward")
    return out, saved


def attention_backward(qkv, out, saved, dout, window):
    """-> dqkv fp16, shaped like qkv, from the upstream gradient dout fp16 [N][T][H*64]."""
    N, T, H, wl, wr = _check(qkv, window, "attention_backward")
    qkv = qkv.contiguous()
    out = half_dev(out, (N, T, H * HEAD_DIM), "out", "attention_backward")
    dout = half_dev(dout, (N, T, H * HEAD_DIM), "dout", "attention_backward")
    lib = _lib.lib()
    if not isinstance(saved, torch.Tensor) or saved.device != qkv.device or saved.dtype != torch.uint8 or saved.dim() != 1 or \
            not saved.is_contiguous() or saved.numel() != lib.bh_attention_train_saved_bytes(N, T, H):
        raise ValueError("attention_backward: `saved` is not what attention_forward returned for N=%d T=%d H=%d" % (N, T, H))
    nbytes = workspace("bh_attention_train_backward_workspace", "attention_backward", N=N, T=T, H=H, window=(wl, wr))
    with torch.cuda.device(qkv.device):
        tab = _table(qkv.device, T)
        dqkv = torch.empty_like(qkv)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=qkv.device)
        _lib.check(lib.bh_attention_train_backward(_lib.ptr(qkv), _lib.ptr(tab), _lib.ptr(out), _lib.ptr(saved), _lib.ptr(dout), N, T, H,
                                                   HEAD_DIM, wl, wr, _lib.ptr(dqkv), _lib.ptr(ws), nbytes, _lib.stream_ptr(qkv.device)),
                   "bh_attention_train_backward")
    return dqkv


def attention(qkv, window):
    """out fp16 [N][T][H*64], differentiable with respect to qkv (fp16 or fp32; fp32 is cast to fp16 and its gradient comes back as fp32)."""
    _, _, _, wl, wr = _check(qkv, window, "attention", dtypes=(torch.float16, torch.float32))

    def forward(qkv16):
        qkv16 = qkv16.contiguous()
        out, saved = attention_forward(qkv16, (wl, wr))
        return out, (qkv16, out, saved)

    def backward(kept, dout, need):
        return (attention_backward(*kept, dout.contiguous(), (wl, wr)),)

    return HalfLayer.apply(forward, backward, qkv)


def mha_module(module, x):
    """A bonito_amd.transformer.model.MultiHeadAttention container applied to x [N][T][D]: Wqkv, rotary + windowed attention, out_proj.
    Gradients land on the container's fp32 parameters (Wqkv.weight, Wqkv.bias if any, out_proj.weight, out_proj.bias if any)."""
    from bonito_amd import train_ops
    window = _mha_check(module, "mha_module")
    _activations(x, module.d_model, "mha_module")
    qkv = train_ops.linear(x, module.Wqkv.weight, module.Wqkv.bias)
    out = attention(qkv, window)
    return train_ops.linear(out, module.out_proj.weight, module.out_proj.bias)


def _mha_check(module, what):
    """What mha_module refuses about the container itself -> its window."""
    from bonito_amd.transformer.model import MultiHeadAttention
    if not isinstance(module, MultiHeadAttention):
        raise ValueError("%s: expected a bonito_amd.transformer.model.MultiHeadAttention container, got %s" % (what, type(module).__name__))
    if module.head_dim != HEAD_DIM:
        raise ValueError("%s: only head_dim %d is served, got %d" % (what, HEAD_DIM, module.head_dim))
    if module.rotary_dim != module.head_dim:
        raise ValueError("%s: rotary_dim must equal head_dim (got %d and %d)" % (what, module.rotary_dim, module.head_dim))
    return _window(module.attn_window, what)


def _activations(x, d_model, what):
    tensors([("x", x)], what)
    if x.dim() != 3 or x.shape[2] != d_model:
        raise ValueError("%s: x must be [N][T][%d], got %s" % (what, d_model, tuple(x.shape)))


def encoder_layer_check(layer, what="encoder_layer"):
    """What encoder_layer refuses about the container itself, in front of any launch: mha_module's refusals, and a dim_feedforward that is
    no multiple of 8. SeqdistModel.forward_train calls it for every layer before its first launch."""
    from bonito_amd.transformer.model import TransformerEncoderLayer
    if not isinstance(layer, TransformerEncoderLayer):
        raise ValueError("%s: expected a bonito_amd.transformer.model.TransformerEncoderLayer container, got %s" % (what, type(layer).__name__))
    _mha_check(layer.self_attn, what)
    F2, D = layer.ff.fc1.weight.shape
    if F2 % 16 != 0 or tuple(layer.ff.fc2.weight.shape) != (layer.self_attn.d_model, F2 // 2) or D != layer.self_attn.d_model:
        raise ValueError("%s: dim_feedforward must be a multiple of 8 (fc1 %s, fc2 %s)"
                         % (what, tuple(layer.ff.fc1.weight.shape), tuple(layer.ff.fc2.weight.shape)))


def _alpha(layer):
    """deepnorm_alpha as a number. It is a buffer (a checkpoint may carry its own value), so it is read from the tensor - once per value:
    reading a device tensor waits for the stream."""
    buf = layer.deepnorm_alpha
    key = (buf._version, buf.data_ptr(), buf.device)
    cached = layer.__dict__.get("_alpha_read")
    if cached is None or cached[0] != key:
        cached = layer.__dict__["_alpha_read"] = (key, float(buf))
    return cached[1]


def encoder_layer(layer, x):
    """A bonito_amd.transformer.model.TransformerEncoderLayer container applied to x [N][T][D] (fp16 or fp32) -> fp16 [N][T][D]:
        x1  = rmsnorm(self_attn(x) + deepnorm_alpha x) norm1.weight
        out = rmsnorm(fc2(swiglu(fc1(x1))) + deepnorm_alpha x1) norm2.weight
    Gradients land on the container's fp32 parameters; deepnorm_alpha is a buffer and gets none."""
    from bonito_amd import train_ops
    encoder_layer_check(layer)
    _activations(x, layer.self_attn.d_model, "encoder_layer")
    alpha = _alpha(layer)
    x1 = train_ops.rmsnorm_residual(mha_module(layer.self_attn, x), x, layer.norm1.weight, alpha, layer.norm1.eps)
    f = train_ops.linear(train_ops.gated_linear(x1, layer.ff.fc1.weight), layer.ff.fc2.weight)
    return train_ops.rmsnorm_residual(f, x1, layer.norm2.weight, alpha, layer.norm2.eps)

"""
One LSTM layer for training on the device: the forward that keeps what the backward needs, the backward, and their autograd
(csrc/lstm_train.hip; the arithmetic is stated in include/bonito_hip.h under bh_lstm_train_forward).

    h, saved = lstm_forward(x, w_ih, w_hh, bias, reverse)                   # x, h fp16 [T][N][H]; the weights fp32 on the device
    dx, dw_ih, dw_hh, db = lstm_backward(x, w_ih, w_hh, h, saved, dh, reverse)
    h = lstm(x, w_ih, w_hh, bias, reverse)                                  # differentiable
    h = lstm_module(layer, x)                                               # a bonito_amd.nn.LSTM container; gradients land on its parameters

torch allocates and orders the streams; every number is computed by libbonito_hip.so. There is no PyTorch fallback: CPU tensors raise
NoTorchCompute, an unsupported shape or dtype raises ValueError before anything is launched.
"""
import torch

from bonito_amd import _lib
from bonito_amd._train import HalfLayer, devices, half_dev, master, tensors, workspace

__all__ = ["lstm_forward", "lstm_backward", "lstm", "lstm_module", "supported_hidden_size"]


def supported_hidden_size(H):
    return 32 <= H <= 1024 and H % 32 == 0


def _check(x, w_ih, w_hh, bias, what):
    named = [("x", x), ("w_ih", w_ih), ("w_hh", w_hh)] + ([("bias", bias)] if bias is not None else [])
    tensors(named, what)
    if x.dim() != 3 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("%s: x must be [T][N][H] with T, N >= 1, got %s" % (what, tuple(x.shape)))
    T, N, H = x.shape
    if not supported_hidden_size(H):
        raise ValueError("%s: hidden size %d is not supported (a multiple of 32 in 32..1024)" % (what, H))
    for name, t in named[1:3]:
        if tuple(t.shape) != (4 * H, H):
            raise ValueError("%s: %s must be [%d][%d] (insize == size), got %s" % (what, name, 4 * H, H, tuple(t.shape)))
        master(t, t.shape, name, what)
    if bias is not None and (tuple(bias.shape) != (4 * H,) or bias.dtype != torch.float32):
        raise ValueError("%s: bias must be float32 [%d], got %s %s" % (what, 4 * H, bias.dtype, tuple(bias.shape)))
    devices(named, what)
    return T, N, H


def lstm_forward(x, w_ih, w_hh, bias=None, reverse=False):
    """-> (h fp16 [T][N][H], saved): `saved` is the opaque byte buffer lstm_backward needs (the gates, c and the fp16 weights)."""
    if isinstance(x, torch.Tensor) and x.dtype != torch.float16:
        raise ValueError("lstm_forward: x must be float16, got %s" % x.dtype)
    T, N, H = _check(x, w_ih, w_hh, bias, "lstm_forward")
    x, w_ih, w_hh = x.contiguous(), w_ih.detach().contiguous(), w_hh.detach().contiguous()
    bias = None if bias is None else bias.detach().contiguous()
    lib = _lib.lib()
    nbytes = workspace("bh_lstm_train_saved_bytes", "lstm_forward", T=T, N=N, H=H)
    with torch.cuda.device(x.device):
        h = torch.empty((T, N, H), dtype=torch.float16, device=x.device)
        saved = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _lib.check(lib.bh_lstm_train_forward(_lib.ptr(x), _lib.ptr(w_ih), _lib.ptr(w_hh), _lib.ptr(bias), T, N, H, int(bool(reverse)),
                                             _lib.ptr(h), _lib.ptr(saved), nbytes, _lib.stream_ptr(x.device)), "bh_lstm_train_forward")
    return h, saved


def lstm_backward(x, w_ih, w_hh, h, saved, dh, reverse=False, need_bias=True):
    """-> (dx fp16 [T][N][H], dw_ih, dw_hh fp32 [4H][H], db fp32 [4H] or None) from the upstream gradient dh fp16 [T][N][H]."""
    T, N, H = _check(x, w_ih, w_hh, None, "lstm_backward")
    x = half_dev(x, (T, N, H), "x", "lstm_backward")
    h = half_dev(h, (T, N, H), "h", "lstm_backward")
    dh = half_dev(dh, (T, N, H), "dh", "lstm_backward")
    w_ih, w_hh = w_ih.detach().contiguous(), w_hh.detach().contiguous()
    lib = _lib.lib()
    if not isinstance(saved, torch.Tensor) or saved.device != x.device or saved.dtype != torch.uint8 or \
            saved.numel() < lib.bh_lstm_train_saved_bytes(T, N, H):
        raise ValueError("lstm_backward: `saved` is not what lstm_forward returned for T=%d N=%d H=%d" % (T, N, H))
    nbytes = lib.bh_lstm_train_backward_workspace(T, N, H)
    with torch.cuda.device(x.device):
        dx = torch.empty((T, N, H), dtype=torch.float16, device=x.device)
        dw_ih = torch.empty((4 * H, H), dtype=torch.float32, device=x.device)
        dw_hh = torch.empty((4 * H, H), dtype=torch.float32, device=x.device)
        db = torch.empty(4 * H, dtype=torch.float32, device=x.device) if need_bias else None
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _lib.check(lib.bh_lstm_train_backward(_lib.ptr(x), _lib.ptr(w_ih), _lib.ptr(w_hh), _lib.ptr(h), _lib.ptr(saved), _lib.ptr(dh), T, N, H,
                                              int(bool(reverse)), _lib.ptr(dx), _lib.ptr(dw_ih), _lib.ptr(dw_hh), _lib.ptr(db), _lib.ptr(ws),
                                              nbytes, _lib.stream_ptr(x.device)), "bh_lstm_train_backward")
    return dx, dw_ih, dw_hh, db


def lstm(x, w_ih, w_hh, bias=None, reverse=False):
    """h fp16 [T][N][H] of one layer, differentiable with respect to x (fp16 or fp32; fp32 is cast to fp16 and its gradient comes back
    as fp32), the two weight matrices and the bias, each where requires_grad is set."""
    if isinstance(x, torch.Tensor) and x.dtype not in (torch.float16, torch.float32):
        raise ValueError("lstm: x must be float16 or float32, got %s" % x.dtype)
    _check(x, w_ih, w_hh, bias, "lstm")
    reverse = bool(reverse)

    def forward(x16, w_ih, w_hh, bias):
        h, saved = lstm_forward(x16, w_ih, w_hh, bias, reverse)
        return h, (x16, w_ih, w_hh, h, saved)

    def backward(kept, dh, need):
        return lstm_backward(*kept, dh, reverse, need_bias=bias is not None and need[3])

    return HalfLayer.apply(forward, backward, x, w_ih, w_hh, bias)


def lstm_module(module, x):
    """A bonito_amd.nn.LSTM container applied to x [T][N][H]: its `reverse` is honoured and b = bias_ih_l0 + bias_hh_l0. Gradients land on
    rnn.weight_ih_l0, rnn.weight_hh_l0 and rnn.bias_ih_l0; the frozen bias_hh_l0 (requires_grad = False) gets none."""
    from bonito_amd.nn import LSTM
    if not isinstance(module, LSTM):
        raise ValueError("lstm_module: expected a bonito_amd.nn.LSTM container, got %s" % type(module).__name__)
    r = module.rnn
    if r.num_layers != 1 or r.bidirectional or r.input_size != r.hidden_size or getattr(r, "proj_size", 0):
        raise ValueError("lstm_module: one layer, one direction, insize == size is what the device layer serves")
    _check(x, r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0 if r.bias else None, "lstm_module")
    bias = r.bias_ih_l0 + r.bias_hh_l0 if r.bias else None
    return lstm(x, r.weight_ih_l0, r.weight_hh_l0, bias, module.reverse)

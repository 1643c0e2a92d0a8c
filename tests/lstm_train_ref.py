"""References of the training LSTM layer (bh_lstm_train_forward / bh_lstm_train_backward, bonito_amd.rnn): the references of
tests/test_gpu_lstm_train.py, pinned by tests/test_lstm_train_ref_cpu.py. Plain torch on the CPU; no import of bonito_amd.

The layer is lstm_ref's: gates i, f, g, o, h_0 = c_0 = 0, `reverse` runs the time loop backwards. Three statements of its gradient:

    written_out   the backward recurrence step by step in fp64, no autograd in it:
                      d_t  = dh_t + da_{t+1} W_hh                 dc_t = dc_{t+1} sig(f_{t+1}) + d_t sig(o) (1 - tanh^2 c_t)
                      da_t = (dc_t tanh(g) sig'(i), dc_t c_{t-1} sig'(f), dc_t sig(i) (1 - tanh^2 g), d_t tanh(c_t) sig'(o))
                      dx_t = da_t W_ih    dW_ih = sum_t da_t^T x_t    dW_hh = sum_t da_t^T h_{t-1}    db = sum_{t,n} da_t
    exact         fp64 autograd through lstm_ref.free_running: what the kernels are measured against
    yardstick     torch.nn.LSTM(H, H).half() on the CPU with its own autograd on the same fp16-valued inputs: the arithmetic the
                  reference trains with, and the measure of how far half-precision training is from `exact` on a given case

dist(a, exact) = max|a - exact| / max|exact| in fp64. The device test requires dist(kernel) <= 2 dist(yardstick) per gradient.
All three return (dx [T][N][H], dW_ih [4H][H], dW_hh [4H][H], db [4H] or None) as float64.
"""
import torch

import lstm_ref

F64 = torch.float64


def _flip(a, reverse):
    return a.flip(0) if reverse else a


def written_out(x, w_ih, w_hh, bias, dh, reverse=False):
    """-> (h, dx, dW_ih, dW_hh, db) float64; h is the forward of the same statement."""
    xs, dhs = _flip(x.to(F64), reverse), _flip(dh.to(F64), reverse)
    wi, wh = w_ih.to(F64), w_hh.to(F64)
    T, N, H = xs.shape
    h = torch.zeros(N, H, dtype=F64)
    c = torch.zeros(N, H, dtype=F64)
    gates, cs, hs = [], [c], [h]
    for t in range(T):
        a = xs[t] @ wi.T + h @ wh.T
        if bias is not None:
            a = a + bias.to(F64)
        ai, af, ag, ao = a.split(H, dim=-1)
        si, sf, tg, so = torch.sigmoid(ai), torch.sigmoid(af), torch.tanh(ag), torch.sigmoid(ao)
        c = sf * c + si * tg
        h = so * torch.tanh(c)
        gates.append((si, sf, tg, so))
        cs.append(c)
        hs.append(h)
    dx = torch.zeros(T, N, H, dtype=F64)
    dwi, dwh, db = torch.zeros(4 * H, H, dtype=F64), torch.zeros(4 * H, H, dtype=F64), torch.zeros(4 * H, dtype=F64)
    da_next = torch.zeros(N, 4 * H, dtype=F64)
    carry = torch.zeros(N, H, dtype=F64)                                  # dc_{t+1} sig(f_{t+1})
    for t in range(T - 1, -1, -1):
        si, sf, tg, so = gates[t]
        tc = torch.tanh(cs[t + 1])
        d = dhs[t] + da_next @ wh
        dc = carry + d * so * (1 - tc * tc)
        da = torch.cat((dc * tg * si * (1 - si), dc * cs[t] * sf * (1 - sf), dc * si * (1 - tg * tg), d * tc * so * (1 - so)), dim=-1)
        dx[t] = da @ wi
        dwi += da.T @ xs[t]
        dwh += da.T @ hs[t]
        db += da.sum(0)
        carry = dc * sf
        da_next = da
    return _flip(torch.stack(hs[1:]), reverse), _flip(dx, reverse), dwi, dwh, (db if bias is not None else None)


def exact(x, w_ih, w_hh, bias, dh, reverse=False):
    """fp64 autograd through lstm_ref.free_running."""
    leaves = [x.to(F64).clone().requires_grad_(), w_ih.to(F64).clone().requires_grad_(), w_hh.to(F64).clone().requires_grad_()]
    b = None
    if bias is not None:
        b = bias.to(F64).clone().requires_grad_()
        leaves.append(b)
    h = lstm_ref.free_running(leaves[0], leaves[1], leaves[2], b, reverse)
    grads = torch.autograd.grad(h, leaves, dh.to(F64))
    return grads[0], grads[1], grads[2], (grads[3] if bias is not None else None)


def half_module(w_ih, w_hh, bias):
    """torch.nn.LSTM(H, H) in half precision on the CPU carrying these weights (bias_hh = 0)."""
    H = w_ih.shape[1]
    m = torch.nn.LSTM(H, H, bias=bias is not None)
    with torch.no_grad():
        m.weight_ih_l0.copy_(w_ih)
        m.weight_hh_l0.copy_(w_hh)
        if bias is not None:
            m.bias_ih_l0.copy_(bias)
            m.bias_hh_l0.zero_()
    return m.half()


def yardstick(x, w_ih, w_hh, bias, dh, reverse=False):
    """torch.nn.LSTM(H, H).half() on the CPU with its own autograd."""
    m = half_module(w_ih.cpu(), w_hh.cpu(), None if bias is None else bias.cpu())
    xs = x.cpu().half().clone().requires_grad_()
    h, _ = m(_flip(xs, reverse))
    _flip(h, reverse).backward(dh.cpu().half())
    db = m.bias_ih_l0.grad.to(F64) if bias is not None else None
    return xs.grad.to(F64), m.weight_ih_l0.grad.to(F64), m.weight_hh_l0.grad.to(F64), db


def dist(a, want):
    """max|a - want| / max|want| in fp64 (0 / 0 = 0; a non-finite a is inf)."""
    a, want = a.detach().to(F64).cpu(), want.detach().to(F64).cpu()
    if not bool(torch.isfinite(a).all()):
        return float("inf")
    err, ref = float((a - want).abs().max()), float(want.abs().max())
    return 0.0 if err == 0.0 else err / ref if ref > 0 else float("inf")


def make_dh(T, N, H, seed=0):
    """dh ~ N(0, 1) rounded to fp16, from a seeded generator."""
    g = torch.Generator().manual_seed(7700 + seed)
    return torch.randn(T, N, H, generator=g).half()


NAMES = ("dx", "dW_ih", "dW_hh", "db")

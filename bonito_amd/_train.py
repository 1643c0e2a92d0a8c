"""What the training layers of bonito_amd.rnn and bonito_amd.train_ops share: the argument checks and the autograd wrapper."""
import torch

from bonito_amd.nn import NoTorchCompute


def tensors(named, what):
    for name, t in named:
        if not isinstance(t, torch.Tensor):
            raise ValueError("%s: %s must be a tensor, got %s" % (what, name, type(t).__name__))


def master(t, shape, name, what):
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s: %s must be %s, got %s" % (what, name, tuple(shape), tuple(t.shape)))
    if t.dtype != torch.float32:
        raise ValueError("%s: %s must be float32 (the master weights), got %s" % (what, name, t.dtype))


def half(t, shape, name, what):
    if t.dtype != torch.float16 or tuple(t.shape) != tuple(shape):
        raise ValueError("%s: %s must be float16 %s, got %s %s" % (what, name, tuple(shape), t.dtype, tuple(t.shape)))


def devices(named, what):
    """Shapes and dtypes are judged first (they are wrong on any device); then every tensor must be on one HIP device."""
    first = named[0][1]
    for name, t in named:
        if t.device.type != "cuda":
            raise NoTorchCompute("%s runs on a HIP device only; %s is a %s tensor" % (what, name, t.device))
        if t.device != first.device:
            raise ValueError("%s: %s is on %s, %s on %s" % (what, name, t.device, named[0][0], first.device))


class HalfLayer(torch.autograd.Function):
    """One layer that computes in fp16: x (fp16 or fp32) is cast to fp16 on entry and its gradient comes back in x's dtype.
    forward(x16, *params) -> (y, the tensors to keep); backward(kept, dy fp16, need) -> (dx, a gradient or None per parameter), `need`
    being needs_input_grad of (x, *params). Gradients nobody asked for are returned as None."""

    @staticmethod
    def forward(ctx, forward, backward, x, *params):
        y, keep = forward(x if x.dtype == torch.float16 else x.to(torch.float16), *params)
        ctx.save_for_backward(*keep)
        ctx.backward_fn, ctx.x_dtype = backward, x.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        need = ctx.needs_input_grad[2:]
        dx, *rest = ctx.backward_fn(ctx.saved_tensors, dy.to(torch.float16), need)
        return (None, None, dx.to(ctx.x_dtype) if need[0] else None) + tuple(g if n else None for g, n in zip(rest, need[1:]))


class HalfLayer2(torch.autograd.Function):
    """HalfLayer with two activations (a sublayer's output a and the residual x beside it): each is cast to fp16 on entry and gets its
    gradient in its own dtype. forward(a16, x16, *params) -> (y, the tensors to keep); backward(kept, dy fp16, need) -> (da, dx, a
    gradient or None per parameter), `need` being needs_input_grad of (a, x, *params)."""

    @staticmethod
    def forward(ctx, forward, backward, a, x, *params):
        a16, x16 = (t if t.dtype == torch.float16 else t.to(torch.float16) for t in (a, x))
        y, keep = forward(a16, x16, *params)
        ctx.save_for_backward(*keep)
        ctx.backward_fn, ctx.dtypes = backward, (a.dtype, x.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        need = ctx.needs_input_grad[2:]
        da, dx, *rest = ctx.backward_fn(ctx.saved_tensors, dy.to(torch.float16), need)
        return (None, None, da.to(ctx.dtypes[0]) if need[0] else None, dx.to(ctx.dtypes[1]) if need[1] else None) \
            + tuple(g if n else None for g, n in zip(rest, need[2:]))

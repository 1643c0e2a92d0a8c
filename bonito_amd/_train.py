"""What the training layers of bonito_amd.rnn, bonito_amd.attn and bonito_amd.train_ops share - the argument checks, the workspace query
and the autograd wrapper - and what the two forward_train plans (crf.model.SeqdistModel, ctc.model.Model) share.

A plan is a list of steps. A step is a callable (h, seed) -> h that applies one device layer with every folding decision already made;
`run` applies them in order. `seed` is the dropout seed of the call, which is drawn after the plan (a refused call draws nothing)."""
import torch

from bonito_amd import _lib, nn as bnn
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


def half_dev(t, shape, name, what):
    """A tensor the caller did not make itself (an upstream gradient, a kept output): on the device, fp16, of this shape -> contiguous."""
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise NoTorchCompute("%s runs on a HIP device only; %s is not a device tensor" % (what, name))
    half(t, shape, name, what)
    return t.contiguous()


def dtype_names(dtypes):
    return " or ".join(str(d).replace("torch.", "") for d in dtypes)


def act_name(activation):
    """None, a name or an activation module -> the name the library knows it by (None stays None)."""
    name = activation if activation is None or isinstance(activation, str) else getattr(activation, "name", type(activation).__name__.lower())
    return "swish" if name == "silu" else name


def unsupported_shape(what, **dims):
    """The refusal of a shape the library returned no workspace size for; a dimension that is a pair (the attention window) reads
    `window (left, right)`."""
    return ValueError("%s: shape %s is not supported"
                      % (what, " ".join(("%s %s" if isinstance(v, tuple) else "%s=%d") % (k, v) for k, v in dims.items())))


def workspace(entry, what, window=(), **dims):
    """The bytes entry point `entry` of the library asks for at these dimensions (its arguments, in order, then the attention window's
    two); 0 is its refusal of the shape."""
    nbytes = getattr(_lib.lib(), entry)(*dims.values(), *window)
    if nbytes == 0:
        raise unsupported_shape(what, **dims, **({"window": window} if window else {}))
    return nbytes


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


# ---- the plans of forward_train ---------------------------------------------------------------------------------------------------------------
def run(steps, h, seed=None):
    for step in steps:
        h = step(h, seed)
    return h


def clamp_after(mods, i):
    """The range of a Clamp directly behind layer i, which layer i fuses, or None."""
    return (float(mods[i + 1].min), float(mods[i + 1].max)) if i + 1 < len(mods) and isinstance(mods[i + 1], bnn.Clamp) else None


def next_compute(mods, i):
    """-> (the layer that consumes layer i's output or None, whether a Permute([2,0,1]) lies between): Permute, Clamp and MakeContiguous
    are folded."""
    tm = False
    for m in mods[i + 1:]:
        if isinstance(m, bnn.Permute):
            tm = tm or list(m.dims) == [2, 0, 1]
        elif not isinstance(m, (bnn.Clamp, bnn.MakeContiguous)):
            return m, tm
    return None, tm


def pad_channels(weight, bias, pad_in, pad_out):
    """Zero input and output channels around a convolution's weight [Cout][Cin][K] and bias: the channels a convolution pair carries
    between them up to a multiple of 8. They stay exactly zero through swish / relu / tanh."""
    if pad_in:
        weight = torch.nn.functional.pad(weight, (0, 0, 0, pad_in))
    if pad_out:
        weight = torch.nn.functional.pad(weight, (0, 0, 0, 0, 0, pad_out))
        bias = None if bias is None else torch.nn.functional.pad(bias, (0, pad_out))
    return weight, bias


def batchnorm_step(bn, *args, pad=0, **kwargs):
    """The step of a torch BatchNorm1d in train mode behind a convolution: train_ops.batchnorm(h, weight, bias, the running statistics,
    momentum, eps, *args, **kwargs) on `pad` zero channels more than bn has, then the batch counter."""
    from bonito_amd import train_ops

    def step(h, seed):
        weight, bias = bn.weight, bn.bias
        if pad:
            weight, bias = torch.nn.functional.pad(weight, (0, pad)), torch.nn.functional.pad(bias, (0, pad))
        h = train_ops.batchnorm(h, weight, bias, bn.running_mean, bn.running_var, bn.momentum, bn.eps, *args, **kwargs)
        if bn.num_batches_tracked is not None:
            bn.num_batches_tracked.add_(1)
        return h
    return step

"""
AdamW with the loss scale and the gradient clip of a mixed-precision training step, computed by csrc/optim.hip (the arithmetic is
stated in include/bonito_hip.h under bh_optim_norm).

    opt = AdamW(model.parameters(), lr=2e-3)
    opt.zero_grad(set_to_none=True)
    opt.scale(model.loss(model.forward_train(x), targets, lengths)).backward()
    opt.step(max_norm=2.0)                   # unscale, gradient norm, overflow check, clip, update, loss-scale rule: no synchronisation
    grad_norm, scale, skipped = opt.last()   # synchronises; for logging

The scalars of a step (loss scale, growth tracker, step, the beta^step products; gradient norm, clip coefficient and the skipped flag
of the last call) live in ``opt.ctl``, a float64 tensor on the device, so nothing of a step waits for the host. There is ONE step
counter for the whole optimizer: a parameter whose gradient appears only later in a run shares the bias correction of the others.

torch allocates and orders the streams; every number is computed by libbonito_hip.so. There is no PyTorch fallback: CPU parameters
raise NoTorchCompute; a dtype, layout or device the kernels do not serve raises ValueError before anything is launched.
"""
import ctypes as C
import math

import numpy as np
import torch

from bonito_amd import _lib
from bonito_amd._train import devices as _devices, tensors as _tensors

__all__ = ["AdamW", "CTL"]

# enum bh_optim_ctl of include/bonito_hip.h (tests/test_optim_ref_cpu.py keeps the two together)
CTL = {"scale": 0, "growth_tracker": 1, "step": 2, "beta1_pow": 3, "beta2_pow": 4, "grad_norm": 5, "clip_coef": 6, "skipped": 7,
       "scale_used": 8, "grad_mul": 9, "bias1": 10, "bias2_sqrt": 11}
CTL_WORDS = 16
KERNEL_VECTOR, KERNEL_SCALAR = 1, 2

# what torch.optim.AdamW keeps in a parameter group besides ours, so that a saved optim_N.tar loads into either class
_TORCH_GROUP_DEFAULTS = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                             decoupled_weight_decay=True)


def beta_power(beta, step):
    """beta^step as the finalise kernel has it: `step` fp64 multiplications, not pow()."""
    value = 1.0
    for _ in range(int(step)):
        value *= beta
    return value


def _pointer_array(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


class AdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=2e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, loss_scale=65536.0, growth_factor=2.0,
                 backoff_factor=0.5, growth_interval=2000):
        what = "optim.AdamW"
        if not 0.0 <= lr < math.inf:
            raise ValueError("%s: lr = %r must be finite and not negative" % (what, lr))
        if not 0.0 <= eps < math.inf:
            raise ValueError("%s: eps = %r must be finite and not negative" % (what, eps))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError("%s: betas %r must lie in [0, 1)" % (what, tuple(betas)))
        if not 0.0 <= weight_decay < math.inf:
            raise ValueError("%s: weight_decay = %r must be finite and not negative" % (what, weight_decay))
        if loss_scale is not None and not (0.0 < loss_scale < math.inf and growth_factor >= 1.0 and 0.0 < backoff_factor <= 1.0
                                           and int(growth_interval) >= 1):
            raise ValueError("%s: loss_scale > 0, growth_factor >= 1, 0 < backoff_factor <= 1 and growth_interval >= 1 are needed "
                             "(%r, %r, %r, %r)" % (what, loss_scale, growth_factor, backoff_factor, growth_interval))
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, **_TORCH_GROUP_DEFAULTS))
        named = [("parameter %d of group %d" % (i, g), p) for g, group in enumerate(self.param_groups) for i, p in enumerate(group["params"])]
        _tensors(named, what)
        for name, p in named:
            if p.dtype != torch.float32:
                raise ValueError("%s: %s must be float32 (the master weights), got %s" % (what, name, p.dtype))
            if not p.is_contiguous():
                raise ValueError("%s: %s is not contiguous" % (what, name))
        _devices(named, what)
        self.device = named[0][1].device
        self.use_scale = loss_scale is not None
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self.param_groups[0]["loss_scale"] = float(loss_scale) if self.use_scale else 1.0
        self.param_groups[0]["growth_tracker"] = 0
        self._chunk = _lib.lib().bh_optim_chunk()
        self._workspace = None
        self._write_ctl(0)

    # ---- the control block --------------------------------------------------------------------------------------------------------------
    def _write_ctl(self, step):
        group = self.param_groups[0]
        words = [0.0] * CTL_WORDS
        words[CTL["scale"]] = float(group["loss_scale"])
        words[CTL["growth_tracker"]] = float(group["growth_tracker"])
        words[CTL["step"]] = float(step)
        words[CTL["beta1_pow"]] = beta_power(group["betas"][0], step)
        words[CTL["beta2_pow"]] = beta_power(group["betas"][1], step)
        self.ctl = torch.tensor(words, dtype=torch.float64).to(self.device)

    def control(self):
        """The control block as a dict of host floats; synchronises."""
        words = self.ctl.cpu().tolist()
        return {name: words[i] for name, i in CTL.items()}

    def scale(self, loss):
        """loss * the loss scale, without a synchronisation (the loss itself when the scale is disabled)."""
        return loss * self.ctl[CTL["scale"]].to(loss.dtype) if self.use_scale else loss

    def last(self):
        """(grad_norm, the loss scale the gradients carried, skipped) of the last step; synchronises."""
        c = self.control()
        return c["grad_norm"], c["scale_used"], bool(c["skipped"])

    # ---- the step -----------------------------------------------------------------------------------------------------------------------
    def _table(self):
        """Per group: the parameters that have a gradient, with their state (made on first sight, as torch does)."""
        what = "optim.AdamW.step"
        groups = []
        for group in self.param_groups:
            rows = []
            for p in group["params"]:
                if not p.requires_grad or p.grad is None:
                    continue
                g = p.grad
                if g.dtype != torch.float32 or g.shape != p.shape or not g.is_contiguous() or g.device != p.device or g.is_sparse:
                    raise ValueError("%s: a gradient must be a contiguous float32 tensor in its parameter's shape and on its device, got %s %s on %s"
                                     % (what, g.dtype, tuple(g.shape), g.device))
                state = self.state[p]
                if "exp_avg" not in state:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if p.numel():
                    rows.append((p.data, g, state["exp_avg"], state["exp_avg_sq"]))
            groups.append(rows)
        return groups

    @torch.no_grad()
    def step(self, max_norm=None, closure=None):
        """One step over every parameter that has a gradient: returns nothing and does not synchronise. max_norm: the global gradient
        norm (of the unscaled gradients) is clipped to it; None or <= 0 = no clip."""
        if closure is not None:
            raise ValueError("optim.AdamW.step: a closure is not supported")
        groups = self._table()
        rows = [r for g in groups for r in g]
        if not rows:
            return
        betas = self.param_groups[0]["betas"]
        for group, grows in zip(self.param_groups, groups):
            if grows and tuple(group["betas"]) != tuple(betas):
                raise ValueError("optim.AdamW.step: every parameter group must have the betas of the first (%r), got %r" % (betas, group["betas"]))
        lib = _lib.lib()
        sizes = (C.c_long * len(rows))(*[r[0].numel() for r in rows])
        nbytes = lib.bh_optim_workspace(sizes, len(rows))
        if nbytes == 0:
            raise ValueError("optim.AdamW.step: %s" % _lib.last_error())
        with torch.cuda.device(self.device):
            if self._workspace is None or self._workspace.numel() < nbytes:
                self._workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            stream = _lib.stream_ptr(self.device)
            _lib.check(lib.bh_optim_norm(_pointer_array([r[1] for r in rows]), sizes, len(rows), _lib.ptr(self.ctl),
                                         float(max_norm) if max_norm is not None else 0.0, int(self.use_scale), self.growth_factor,
                                         self.backoff_factor, self.growth_interval, float(betas[0]), float(betas[1]),
                                         _lib.ptr(self._workspace), self._workspace.numel(), stream), "bh_optim_norm")
            for group, grows in zip(self.param_groups, groups):
                if not grows:
                    continue
                gsizes = (C.c_long * len(grows))(*[r[0].numel() for r in grows])
                _lib.check(lib.bh_optim_update(*[_pointer_array([r[k] for r in grows]) for k in range(4)], gsizes, len(grows),
                                               _lib.ptr(self.ctl), float(group["lr"]), float(betas[0]), float(betas[1]), float(group["eps"]),
                                               float(group["weight_decay"]), stream), "bh_optim_update")

    # ---- checkpoints: the layout of torch.optim.AdamW ------------------------------------------------------------------------------------
    def state_dict(self):
        """The state dict of torch.optim.AdamW (step, exp_avg, exp_avg_sq per parameter) with loss_scale and growth_tracker as extra keys
        of param_groups[0]; synchronises."""
        c = self.control()
        for state in self.state.values():
            if "exp_avg" in state:
                state["step"] = torch.tensor(c["step"], dtype=torch.float32)
        self.param_groups[0]["loss_scale"] = c["scale"]
        self.param_groups[0]["growth_tracker"] = int(c["growth_tracker"])
        packed = super().state_dict()
        for group in packed["param_groups"]:           # a scheduler leaves numpy scalars in lr: plain numbers load with weights_only
            for key, value in group.items():
                if isinstance(value, np.generic):
                    group[key] = value.item()
        return packed

    def load_state_dict(self, state_dict):
        """Takes a state dict of this class or of torch.optim.AdamW (no loss scale there: the current one is kept)."""
        keep = {k: self.param_groups[0][k] for k in ("loss_scale", "growth_tracker")}
        super().load_state_dict(state_dict)
        for k, v in keep.items():
            self.param_groups[0].setdefault(k, v)
        steps = {float(s["step"]) for s in self.state.values() if "step" in s}
        if len(steps) > 1:
            raise ValueError("optim.AdamW.load_state_dict: the parameters are at different steps (%s); this optimizer has one step counter"
                             % sorted(steps))
        for p, state in self.state.items():
            for key in ("exp_avg", "exp_avg_sq"):
                if key in state and (state[key].dtype != torch.float32 or state[key].shape != p.shape or state[key].device != p.device):
                    raise ValueError("optim.AdamW.load_state_dict: %s must be float32 in its parameter's shape and on its device" % key)
                if key in state:
                    state[key] = state[key].contiguous()
            if "step" in state:
                state["step"] = torch.as_tensor(state["step"], dtype=torch.float32).cpu()
        self._write_ctl(int(steps.pop()) if steps else 0)

"""
Learning-rate schedules of a training run: each factory returns ``f(optimizer, steps_per_epoch, epochs, last_epoch) -> LambdaLR``, the
signature ``Trainer`` calls (the names, arguments and values of the reference's bonito/schedule.py; tests/golden/schedule_cases.json
holds values recorded from it). A schedule is a function of t = step / total_steps in [0, 1] that multiplies the optimizer's lr.
"""
import math

import numpy as np
from torch.optim.lr_scheduler import LambdaLR

__all__ = ["linear_warmup_cosine_decay", "linear_warmup_const_inverse_sqrt_decay", "linear_cooldown", "const_schedule", "linear_schedule",
           "cosine_decay_schedule", "piecewise_schedule", "inverse_sqrt_decay_schedule", "func_scheduler"]


# ---- functions of t -----------------------------------------------------------------------------------------------------------------------
def const_schedule(y):
    return lambda t: y


def linear_schedule(y0, y1):
    return lambda t: y0 + (y1 - y0) * t


def cosine_decay_schedule(y0, y1):
    return lambda t: y1 + 0.5 * (y0 - y1) * (np.cos(t * np.pi) + 1.0)


def inverse_sqrt_decay_schedule(scale):
    return lambda t: 1.0 / math.sqrt(1 + scale * t)


def piecewise_schedule(knots, funcs):
    """funcs[i] over [knots[i-1], knots[i]] (0 and 1 at the ends), each seeing its own interval as [0, 1]; a knot belongs to the
    piece on its left."""
    def f(t):
        i = int(np.searchsorted(knots, t))
        lo = knots[i - 1] if i > 0 else 0.0
        hi = knots[i] if i < len(knots) else 1.0
        return funcs[i]((t - lo) / (hi - lo))
    return f


def func_scheduler(optimizer, func, total_steps, warmup_steps=None, warmup_ratio=0.1, start_step=0):
    """LambdaLR of func((step + start_step) / total_steps), behind a linear warm-up from warmup_ratio * func(0) when warmup_steps is set."""
    if warmup_steps:
        y0 = func(0.0)
        func = piecewise_schedule([warmup_steps / total_steps], [linear_schedule(warmup_ratio * y0, y0), func])
    return LambdaLR(optimizer, lambda step: func((step + start_step) / total_steps))


# ---- the factories a config's [lr_scheduler] names ---------------------------------------------------------------------------------------
def linear_warmup_cosine_decay(end_ratio=0.01, warmup_steps=500, **kwargs):
    def make(optimizer, steps_per_epoch, epochs, last_epoch):
        return func_scheduler(optimizer, cosine_decay_schedule(1.0, end_ratio), epochs * steps_per_epoch, warmup_steps=warmup_steps,
                              start_step=last_epoch * steps_per_epoch)
    return make


def linear_warmup_const_inverse_sqrt_decay(warmup_steps=1000, decay_start_epoch=10, decay_scale=1.0, linear_cooldown_n_epochs=0,
                                           linear_cooldown_end_ratio=0.0, **kwargs):
    def make(optimizer, steps_per_epoch, epochs, last_epoch):
        start_step, total_steps = steps_per_epoch * last_epoch, steps_per_epoch * epochs
        decay = inverse_sqrt_decay_schedule(decay_scale * (epochs - decay_start_epoch - linear_cooldown_n_epochs))
        func = piecewise_schedule(
            [warmup_steps / total_steps, decay_start_epoch / epochs, (epochs - linear_cooldown_n_epochs) / epochs],
            [linear_schedule(0.0, 1.0), const_schedule(1.0), decay, linear_schedule(decay(1.0), linear_cooldown_end_ratio)])
        return LambdaLR(optimizer, lambda step: func((step + start_step) / total_steps))
    return make


def linear_cooldown(end_ratio=0.0, **kwargs):
    def make(optimizer, steps_per_epoch, epochs, last_epoch):
        return func_scheduler(optimizer, linear_schedule(1.0, end_ratio), epochs * steps_per_epoch, start_step=0)
    return make

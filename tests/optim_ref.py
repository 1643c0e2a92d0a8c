"""The optimizer step of csrc/optim.hip (include/bonito_hip.h: bh_optim_norm, bh_optim_update) stated twice: in fp64, which is exact
for every purpose of the tests, and in numpy fp32 operation by operation, which gives the bytes the update kernel must write.

A control block is a dict of Python floats under the names of bonito_amd.optim.CTL. `defect` plants one wrong reading of the
definition into the fp64 statement (tests/test_optim_ref_cpu.py shows that the comparison against torch rejects each)."""
import math

import numpy as np

DEFECTS = ("coupled_weight_decay", "no_bias_correction", "eps_inside_sqrt", "clip_without_1e-6", "step_on_skip", "no_unscale")


def new_control(loss_scale=65536.0):
    return dict(scale=float(loss_scale), growth_tracker=0.0, step=0.0, beta1_pow=1.0, beta2_pow=1.0, grad_norm=0.0, clip_coef=0.0,
                skipped=0.0, scale_used=0.0, grad_mul=0.0, bias1=0.0, bias2_sqrt=0.0)


def sum_of_squares(grads):
    """fp64 sum of g^2 over a list of arrays. inf / nan propagate, and a square that overflows fp32 makes the sum inf: the kernel squares
    in fp32, and the definition counts that as an overflow."""
    grads = [np.asarray(g) for g in grads]
    with np.errstate(all="ignore"):
        total = float(sum(np.sum(g.astype(np.float64) ** 2) for g in grads))
        if any(g.dtype == np.float32 and not np.isfinite(g * g).all() for g in grads) and total == total:
            return float("inf")
    return total


def finalise(ctl, sum_sq, max_norm=None, use_scale=True, growth=2.0, backoff=0.5, growth_interval=2000, betas=(0.9, 0.999), defect=None):
    """The finalise launch: -> the next control block."""
    c = dict(ctl)
    scale = c["scale"] if use_scale else 1.0
    skipped = not math.isfinite(sum_sq)
    norm = (math.sqrt(sum_sq) if sum_sq == sum_sq and sum_sq >= 0 else float("nan")) / scale
    if defect == "no_unscale":
        norm = norm * scale
    c.update(grad_norm=norm, skipped=float(skipped), scale_used=scale)
    if not skipped or defect == "step_on_skip":
        c["step"] += 1.0
        c["beta1_pow"] *= betas[0]
        c["beta2_pow"] *= betas[1]
    if not skipped:
        eps = 0.0 if defect == "clip_without_1e-6" else 1e-6
        clip = min(1.0, max_norm / (norm + eps)) if max_norm is not None and max_norm > 0 else 1.0
        c.update(clip_coef=clip, grad_mul=clip if defect == "no_unscale" else clip / scale, bias1=1.0 - c["beta1_pow"],
                 bias2_sqrt=math.sqrt(1.0 - c["beta2_pow"]))
    else:
        c.update(clip_coef=0.0, grad_mul=0.0)
    if use_scale:
        if skipped:
            c.update(scale=scale * backoff, growth_tracker=0.0)
        elif c["growth_tracker"] + 1.0 == float(growth_interval):
            c.update(scale=scale * growth, growth_tracker=0.0)
        else:
            c["growth_tracker"] += 1.0
    return c


def adamw_fp64(p, g, m, v, ctl, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, defect=None):
    """The update launch in fp64 from the control block finalise left: -> (p, m, v); the inputs are not written."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    if ctl["skipped"]:
        return p.copy(), m.copy(), v.copy()
    b1, b2 = betas
    gs = g * ctl["grad_mul"]
    if defect == "coupled_weight_decay":
        gs = gs + weight_decay * p
    else:
        p = p * (1.0 - lr * weight_decay)
    m = b1 * m + (1.0 - b1) * gs
    v = b2 * v + (1.0 - b2) * gs * gs
    bias1, bias2_sqrt = (1.0, 1.0) if defect == "no_bias_correction" else (ctl["bias1"], ctl["bias2_sqrt"])
    denom = np.sqrt(v / bias2_sqrt ** 2 + eps) if defect == "eps_inside_sqrt" else np.sqrt(v) / bias2_sqrt + eps
    return p - (lr / bias1) * (m / denom), m, v


def adamw_fp32(p, g, m, v, ctl, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01):
    """The update launch as the kernel computes it: every scalar rounded to fp32 once, every operation rounded to fp32, divide and
    square root correctly rounded (numpy's are). -> (p, m, v) float32; the inputs are not written."""
    f = np.float32
    p, g, m, v = (np.array(a, dtype=f, copy=True) for a in (p, g, m, v))
    if ctl["skipped"]:
        return p, m, v
    grad_mul, decay = f(ctl["grad_mul"]), f(1.0 - lr * weight_decay)
    b1, one_minus_b1, b2, one_minus_b2 = f(betas[0]), f(1.0 - betas[0]), f(betas[1]), f(1.0 - betas[1])
    bias2_sqrt, eps, step_size = f(ctl["bias2_sqrt"]), f(eps), f(lr / ctl["bias1"])
    with np.errstate(all="ignore"):
        gs = g * grad_mul
        p = p * decay
        m = b1 * m + one_minus_b1 * gs
        v = b2 * v + (one_minus_b2 * gs) * gs
        denom = np.sqrt(v) / bias2_sqrt + eps
        p = p - step_size * (m / denom)
    assert p.dtype == m.dtype == v.dtype == f
    return p, m, v


def step_fp64(params, grads, ms, vs, ctl, lr, max_norm=None, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, use_scale=True,
              growth=2.0, backoff=0.5, growth_interval=2000, defect=None):
    """A whole step over lists of arrays in fp64: -> (params, ms, vs, control block)."""
    c = finalise(ctl, sum_of_squares(grads), max_norm, use_scale, growth, backoff, growth_interval, betas, defect)
    out = [adamw_fp64(p, g, m, v, c, lr, betas, eps, weight_decay, defect) for p, g, m, v in zip(params, grads, ms, vs)]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], c


def ulp_distance(a, b):
    """Largest distance between two float32 arrays in units in the last place (both finite)."""
    a, b = (np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64) for x in (a, b))
    a, b = (np.where(x < 0, -(x & 0x7FFFFFFF), x) for x in (a, b))
    return int(np.abs(a - b).max()) if a.size else 0

"""tests/linear_ref.py is itself under test (no GPU): `want` against a naive triple loop for every option, the rotary convention against
bh_rotary_table + the rotate_half form of the reference model, the bound against a float32 emulation of a CORRECT kernel (zero elements
over it, on every shape class of tests/test_gpu_linear.py that fits the CPU) and against planted defects (each must fail)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import linear_ref as lr
from linear_ref import Call

INF = float("inf")
QS = 0.125 * math.log2(math.e)
S5 = dict(scale=5.0, lo=-4.5, hi=4.5)


def _naive(c, t):
    """Triple loop in Python floats (fp64), straight from the description of the operation."""
    X, W = t["X"].double().tolist(), t["W"].double().tolist()
    bias = t["bias"].double().tolist() if c.bias else [0.0] * c.N
    res = t["res"].double().tolist() if c.res_scale is not None else None
    rs = float(np.float32(c.res_scale)) if c.res_scale is not None else 0.0
    sw = lambda v: v / (1.0 + math.exp(-v))
    act = {0: lambda v: v, 1: sw, 2: math.tanh, 3: lambda v: max(v, 0.0)}[c.act]
    rows = {}
    for m in range(c.M):
        z = []
        for n in range(c.N):
            s = 0.0
            for k in range(c.K):
                s += X[m][k] * W[n][k]
            s += bias[n]
            if res is not None:
                s += rs * res[m][n]
            z.append(s)
        if c.rot is not None:
            T, q = c.rot
            q = float(np.float32(q))
            D = c.N // 3
            cs = t["cs"].double().tolist()
            y = list(z)
            for h in range(2 * D // 64):
                for i in range(32):
                    co, si = cs[m % T][i]
                    a, b = z[64 * h + i], z[64 * h + 32 + i]
                    f = q if 64 * h < D else 1.0
                    y[64 * h + i], y[64 * h + 32 + i] = (a * co - b * si) * f, (a * si + b * co) * f
        elif c.gated:
            y = [z[2 * j] * sw(z[2 * j + 1]) for j in range(c.N // 2)]
        else:
            y = [act(v) for v in z]
        y = [min(max(v * float(np.float32(c.scale)), c.lo), c.hi) for v in y]
        div, s_hi, s_lo, lim = c.row
        if div > 0:
            if lim > 0 and m % div >= lim:
                continue
            rows[(m // div) * s_hi + (m % div) * s_lo] = (m, y)
        else:
            rows[m] = (m, y)
    return rows


SMALL = [
    Call(5, 16, 16), Call(5, 6, 24, bias=False), Call(4, 16, 8, act=1), Call(4, 16, 8, act=2, **S5), Call(4, 16, 8, act=3, scale=5.0),
    Call(4, 16, 8, act=1, lo=-0.1, hi=0.4), Call(6, 32, 16, gated=1), Call(6, 32, 16, gated=1, bias=False, **S5),
    Call(5, 16, 16, res_scale=2.4494897), Call(5, 16, 16, res_scale=1.0, act=2, ldres=24), Call(5, 32, 8, res_scale=2.4494897, gated=1),
    Call(12, 8, 16, row=(4, 1, 3, 3)), Call(12, 8, 16, row=(4, 1, 3, 3), res_scale=1.0), Call(7, 192, 16, rot=(3, QS)),
    Call(5, 16, 16, ldx=24, ldw=40, ldo=24), Call(9, 384, 8, rot=(4, QS), bias=False),
]


@pytest.mark.parametrize("c", SMALL, ids=repr)
def test_want_is_the_naive_triple_loop(c):
    t = lr.make_inputs(c, "cpu", 1)
    want, bound = lr.reference(c, t["X"], t["W"], t["bias"], t["res"], t["cs"])
    orow, live = c.row_map()
    naive = _naive(c, t)
    assert sorted(naive) == sorted(orow[live].tolist())                     # the set of rows written
    for o, (m, y) in naive.items():
        assert int(orow[m]) == o
        np.testing.assert_allclose(want[m].numpy(), np.array(y), rtol=1e-12, atol=1e-13)
    assert (bound > 0).all() and torch.isfinite(bound).all()
    w = c.writable()
    assert int(w.sum()) == len(naive) * c.ncol and not w[:, c.ncol:].any() and not w[c.rows_addressable():].any()


def test_ulp_fp16():
    v = torch.tensor([0.0, 1e-9, 2.0 ** -14, 0.75, 1.0, 1.5, 2.0, 4.5, -1000.0, 65504.0], dtype=torch.float64)
    want = [2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -11, 2.0 ** -10, 2.0 ** -10, 2.0 ** -9, 2.0 ** -8, 0.5, 32.0]
    assert lr.ulp_fp16(v).tolist() == want
    for x in (0.75, 1.0, 4.5, 1000.0):                                     # the spacing numpy's fp16 has there
        assert float(np.spacing(np.float16(x))) == float(lr.ulp_fp16(torch.tensor([x], dtype=torch.float64))[0])


def test_rotary_convention_is_the_reference_models():
    """linear_ref.rotary_table is bh_rotary_table, and `want` of a rotary call is apply_rotary of the reference model restated:
    x * cos + rotate_half(x) * sin with rotate_half(x) = (-x2, x1), non-interleaved halves, q scaled afterwards."""
    from bonito_amd import _lib
    T = 300
    tab = np.zeros((T, 32, 2), np.float32)
    assert _lib.lib().bh_rotary_table(T, 64, tab.ctypes.data_as(C.c_void_p)) == 0
    mine = lr.rotary_table(T).numpy()
    assert np.abs(mine - tab).max() < 4e-5          # fp32 sin / cos of arguments up to 300 rad: the argument's own rounding (300 x 2^-24)
    c = Call(23, 384, 16, rot=(5, QS))
    t = lr.make_inputs(c, "cpu", 2)
    want, _ = lr.reference(c, t["X"], t["W"], t["bias"], t["res"], t["cs"])
    z = t["X"][:, :16].double() @ t["W"][:, :16].double().T + t["bias"].double()
    pos = torch.arange(23) % 5
    cos = torch.cat((t["cs"][pos, :, 0], t["cs"][pos, :, 0]), dim=-1).double()[:, None, :]       # [m][1][64]
    sin = torch.cat((t["cs"][pos, :, 1], t["cs"][pos, :, 1]), dim=-1).double()[:, None, :]
    qk = z[:, :256].reshape(23, 4, 64)
    rot_half = torch.cat((-qk[..., 32:], qk[..., :32]), dim=-1)
    qk = (qk * cos + rot_half * sin).reshape(23, 256)
    qk[:, :128] *= float(np.float32(QS))
    np.testing.assert_allclose(want.numpy(), torch.cat((qk, z[:, 256:]), dim=1).numpy(), rtol=1e-12, atol=1e-13)


# the shape classes of tests/test_gpu_linear.py, big ones capped at a few thousand rows
R = 2.4494897
CLASSES = [
    # K tails (v1) and the feature / token edges
    Call(300, 136, 72), Call(129, 77, 200), Call(15, 5, 8), Call(127, 80, 1000, act=1), Call(128, 8, 40, bias=False), Call(1, 128, 24),
    Call(300, 136, 16, act=2, **S5), Call(64, 77, 1000),
    # v2
    Call(300, 136, 96, act=3), Call(129, 80, 2048), Call(127, 77, 160, act=1, scale=5.0), Call(15, 5, 32), Call(128, 128, 64, gated=1),
    # v3
    Call(600, 320, 192, act=1), Call(513, 1040, 64, bias=False), Call(300, 272, 512, act=2, **S5),
    # v5
    Call(1007, 768, 384), Call(257, 256, 2048, act=2, **S5), Call(2009, 1536, 640, gated=1, bias=False), Call(255, 256, 1024, act=1),
    Call(1007, 256, 512, res_scale=R),
    # epilogues
    Call(300, 136, 72, act=1, lo=-0.1, hi=2.0), Call(300, 136, 72, act=3, scale=5.0, bias=False), Call(300, 136, 72, act=2, res_scale=R),
    Call(300, 136, 72, act=1, res_scale=1.0, bias=False), Call(300, 144, 72, gated=1, res_scale=R), Call(300, 144, 96, gated=1, **S5),
    # rotary
    Call(37, 192, 64, rot=(17, QS)), Call(603, 384, 128, rot=(300, QS), bias=False), Call(515, 1536, 512, rot=(256, QS)),
    Call(5, 192, 64, rot=(1, QS)),
    # row remap
    Call(7 * 16, 64, 64, row=(16, 1, 7, 11)), Call(3 * 256, 256, 384, act=2, row=(256, 1, 3, 251), **S5),
    Call(5 * 48, 77, 72, row=(48, 1, 5, 1)), Call(7 * 16, 64, 64, row=(16, 1, 7, 11), res_scale=R),
    # leading dimensions
    Call(129, 136, 72, ldx=80, ldw=96, ldo=144, res_scale=R, ldres=144), Call(129, 144, 96, gated=1, ldo=80),
    Call(300, 256, 384, ldx=392, ldw=408, ldo=264), Call(129, 77, 200, ldx=208, ldw=224),
]


@pytest.mark.parametrize("c", CLASSES, ids=repr)
def test_bound_admits_a_correct_kernel(c):
    """fp32 accumulation in shuffled 8-half chunks, fp32 epilogue, one rounding: ZERO elements over the bound, every guard intact."""
    t = lr.make_inputs(c, "cpu", 7)
    for seed in (0, 1):
        buf = lr.emulate(c, t, c.alloc_out("cpu"), seed=seed)
        r = lr.verify(c, t, buf, slab=1024)
        assert r["bad"] == 0 and r["lost"] == 0 and r["worst"] < 1.0, lr.message(c, r, "correct emulation")
        assert r["worst"] > 0.0


PLANTED = [
    ("drop_chunk", Call(300, 136, 72)), ("drop_chunk", Call(129, 80, 2048)), ("drop_chunk", Call(257, 256, 2048, act=2, **S5)),
    ("k_tail", Call(300, 136, 72)), ("k_tail", Call(129, 77, 200, ldx=208, ldw=224)),
    ("bias_next", Call(300, 136, 72)), ("bias_next", Call(257, 256, 2048, act=2, **S5)),
    ("res_next", Call(300, 136, 72, act=2, res_scale=R)), ("no_res_scale", Call(300, 136, 72, act=2, res_scale=R)),
    ("no_res_scale", Call(1007, 256, 512, res_scale=R)), ("res_outrow", Call(7 * 16, 64, 64, row=(16, 1, 7, 11), res_scale=R)),
    ("rot_sign", Call(37, 192, 64, rot=(17, QS))), ("rot_pos", Call(37, 192, 64, rot=(17, QS))), ("rot_qk", Call(37, 192, 64, rot=(17, QS))),
    ("rot_pos", Call(515, 1536, 512, rot=(256, QS))), ("rot_qk", Call(515, 1536, 512, rot=(256, QS))),
    ("swap_gate", Call(128, 128, 64, gated=1)), ("swap_gate", Call(300, 144, 72, gated=1, res_scale=R)),
    ("scale_first", Call(300, 136, 16, act=2, **S5)), ("clamp_first", Call(300, 136, 16, act=2, **S5)),
    ("scale_first", Call(127, 77, 160, act=1, scale=5.0)), ("clamp_first", Call(257, 256, 2048, act=2, **S5)),
    ("store16", Call(129, 77, 200)), ("store16", Call(15, 5, 8)), ("store16", Call(5 * 48, 77, 72, row=(48, 1, 5, 1))),
    ("store_dropped", Call(7 * 16, 64, 64, row=(16, 1, 7, 11))), ("store_dropped", Call(3 * 256, 256, 384, act=2, row=(256, 1, 3, 251), **S5)),
]


@pytest.mark.parametrize("defect,c", PLANTED, ids=lambda v: v if isinstance(v, str) else repr(v))
def test_bound_rejects_a_subtly_wrong_kernel(defect, c):
    assert any(repr(c) == repr(k) for k in CLASSES)                 # the inputs of the admitted cases: what the GPU tests use
    t = lr.make_inputs(c, "cpu", 7)
    r = lr.verify(c, t, lr.emulate(c, t, c.alloc_out("cpu"), defect=defect), slab=1024)
    assert r["bad"] > 0 or r["lost"] > 0, "the planted defect %s passed: %s" % (defect, lr.message(c, r))
    if defect in ("store16", "store_dropped"):
        assert r["lost"] > 0                                        # guard bytes gone: what the sentinel check is for
    print("%s: %s" % (defect, lr.message(c, r)))


def test_every_defect_is_planted_somewhere():
    assert sorted(set(d for d, _ in PLANTED)) == sorted(lr.DEFECTS)

"""tests/lstm_ref.py pinned on the CPU: its fp64 recurrence against a scalar triple loop, and its bound against a float32 emulation of a
correct kernel (lstm_cell() spelled as csrc/lstm.hip spells it, fp32 accumulation in two orders, h rounded to fp16 before it is fed
back, with and without the fp16 gate tensor G): ZERO elements over the bound on every data class, both directions, T = 400 - and at least
one element over it for each of fourteen planted defects, on the data class named beside the defect."""
import math

import numpy as np
import pytest
import torch

import lstm_ref as lr

F32 = np.float32
T_LONG, N, H = 400, 32, 64


# ---- the scalar definition -------------------------------------------------------------------------------------------------------
def _naive(x, w_ih, w_hh, bias, reverse, h_pub=None):
    """Triple loop in Python floats (fp64). h_pub given: teacher forced from it. -> h [T][N][H] nested lists."""
    T, n, h = x.shape
    sig = lambda v: 1.0 / (1.0 + math.exp(-v))
    out = [[[0.0] * h for _ in range(n)] for _ in range(T)]
    for b in range(n):
        hp, c = [0.0] * h, [0.0] * h
        for s in range(T):
            t = T - 1 - s if reverse else s
            if h_pub is not None and s > 0:
                hp = [float(h_pub[t + (1 if reverse else -1), b, k]) for k in range(h)]
            a = []
            for r in range(4 * h):
                acc = float(bias[r]) if bias is not None else 0.0
                for k in range(h):
                    acc += float(x[t, b, k]) * float(w_ih[r, k]) + hp[k] * float(w_hh[r, k])
                a.append(acc)
            for u in range(h):
                c[u] = sig(a[h + u]) * c[u] + sig(a[u]) * math.tanh(a[2 * h + u])
                out[t][b][u] = sig(a[3 * h + u]) * math.tanh(c[u])
            hp = list(out[t][b])
    return torch.tensor(out, dtype=torch.float64)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("cls", ["typical", "saturating"])
def test_reference_is_the_scalar_triple_loop(cls, reverse):
    x, w_ih, w_hh, bias = lr.make_case(cls, 5, 2, 8, seed=3)
    free = lr.free_running(x, w_ih, w_hh, bias, reverse)
    assert torch.allclose(free, _naive(x, w_ih, w_hh, bias, reverse), rtol=0, atol=1e-13)
    pub = (free + 0.01 * torch.randn(free.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)).half()
    want, bound = lr.teacher_forced(x, w_ih, w_hh, bias, pub, reverse)
    assert torch.allclose(want, _naive(x, w_ih, w_hh, bias, reverse, h_pub=pub), rtol=0, atol=1e-13)
    assert (bound > 0).all() and torch.isfinite(bound).all()
    # fed its own (rounded) output, the teacher-forced reference is the free-running one up to that rounding
    want2, bound2 = lr.teacher_forced(x, w_ih, w_hh, bias, free.half(), reverse)
    assert ((want2 - free).abs() <= 8 * 2.0 ** -11).all()


def test_ulp_fp16_and_classes():
    v = torch.tensor([0.0, 1.0, 0.75, 1e-7, 30.0], dtype=torch.float64)
    assert lr.ulp_fp16(v).tolist() == [2.0 ** -24, 2.0 ** -10, 2.0 ** -11, 2.0 ** -24, 2.0 ** -6]
    x, w_ih, w_hh, bias = lr.make_case("saturating", 3, 16, 64)
    b = bias.view(4, 64)
    for gate, mag in ((0, 30.0), (1, 30.0), (2, 15.0), (3, 30.0)):
        assert (b[gate] == mag).any() and (b[gate] == -mag).any()
    assert torch.equal(w_ih, w_ih.half().float()) and w_ih.abs().max() <= 1 / 8 and x.abs().max() <= 4
    xr = lr.make_case("typical", 3, 16, 64, replicate=True)[0]
    assert all(torch.equal(xr[:, 0], xr[:, n]) for n in range(16))
    assert lr.make_case("zeros", 3, 16, 64)[3] is None


# ---- float32 emulation of the kernel ---------------------------------------------------------------------------------------------
def _fma(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)       # a*b exact in fp64: one rounding + a double rounding far below u


def _cell(ai, af, ag, ao, c, defect=None):
    """lstm_cell() of csrc/lstm.hip, operation by operation in float32. -> (h, c')"""
    one, two = F32(1), F32(2)
    gl = F32(2.5) if defect == "g_clamp" else F32(12.5)
    clip = (lambda v: v) if defect == "no_clamp" else (lambda v: np.clip(v, F32(-25), F32(25)))
    with np.errstate(all="ignore"):
        ei, ef, eo = np.exp(-clip(ai)), np.exp(-clip(af)), np.exp(-clip(ao))
        eg = np.exp(-two * np.clip(ag, -gl, gl))
        didg = (one + ei) * (one + eg)
        df = one + ef
        num = _fma(c, didg, (one - eg) * df)
        c = num * (one / (df * didg))
        ec = np.exp(-two * np.clip(c, F32(-12.5), F32(12.5)))
        if defect == "tanh_approx":
            th = ((one - ec) / (one + ec) + F32(1e-3) * np.sin(F32(4) * c)).astype(F32)       # |error| <= 1e-3, none at c = 0
            hv = th * (one / (one + eo))
        else:
            hv = (one - ec) * (one / ((one + ec) * (one + eo)))
        hv = np.where(np.abs(hv) <= one, hv, F32(0))          # (NaN compares false)
    return hv.astype(F32), c.astype(F32)


def _slices(v, w, order, drop=None):
    """sum over 32-wide K-slices of v [N][K] @ w[4H][K]^T in float32, slice order by `order`."""
    ks = list(range(v.shape[1] // 32))
    acc = np.zeros((v.shape[0], w.shape[0]), F32)
    for k in (ks if order == 0 else ks[::-1]):
        if k != drop:
            acc = acc + v[:, 32 * k:32 * k + 32] @ w[:, 32 * k:32 * k + 32].T
    return acc


def emulate(case, reverse, order=0, gemm=False, defect=None):
    """-> the fp16 h [T][N][H] a kernel of that description publishes (torch)."""
    x, w_ih, w_hh, bias = case
    xs = x.float().numpy()
    T, n, h = xs.shape
    wi, wh = w_ih.numpy(), w_hh.numpy()
    b = np.zeros(4 * h, F32) if bias is None else bias.numpy().copy()
    if defect == "no_bias_gate":
        b[h:2 * h] = 0
    if defect == "swap_if":                                  # units 8..15: gate rows i <-> f
        for w in (wi, wh, b):
            w[8:16], w[h + 8:h + 16] = w[h + 8:h + 16].copy(), w[8:16].copy()
    run_rev = reverse and defect != "forwards"
    out = np.full((T, n, h), np.nan, np.float16)
    hp = np.zeros((n, h), F32)
    hpp = np.zeros((n, h), F32)
    c = np.zeros((n, h), F32)
    for s in range(T):
        t = T - 1 - s if run_rev else s
        gx = _slices(xs[t], wi, order, drop=0 if defect == "drop_x_slice" else None)
        hin = hp
        if defect == "stale_h" and s == 7:                   # one slice of 32 reads h_{t-2}
            hin = hp.copy()
            hin[:, :32] = hpp[:, :32]
        gh = _slices(hin, wh, order, drop=1 if defect == "drop_h_slice" else None)
        if gemm:
            G = (gx + b).astype(np.float16).astype(F32)
            a = gh + (G + G if defect == "g_twice" else G)
        elif order == 0:
            a = (b + gx) + gh
            if defect == "g_twice":
                a = a + (b + gx)
        else:
            a = (gh + gx) + b
            if defect == "g_twice":
                a = a + (b + gx)
        if defect == "c_reset" and s == 4:
            c = np.zeros_like(c)
        hv, c = _cell(a[:, :h], a[:, h:2 * h], a[:, 2 * h:3 * h], a[:, 3 * h:], c, defect)
        if defect == "c_neighbour" and s == 5:               # ring 1 carries ring 0's cell state from here
            c[16:32] = c[0:16]
        h16 = hv.astype(np.float16)
        if not (defect == "last_step" and s == T - 1):
            out[t] = h16
        hpp, hp = hp, h16.astype(F32)
    if defect == "column_shift":
        out = np.roll(out, 16, axis=1)
    return torch.from_numpy(out)


def _ratio(case, reverse, got, gemm):
    x, w_ih, w_hh, bias = case
    want, bound = lr.teacher_forced(x, w_ih, w_hh, bias, got, reverse, gemm=gemm)
    return lr.worst(got, want, bound)


_CASES = {}


def _case(cls):
    if cls not in _CASES:
        _CASES[cls] = lr.make_case(cls, T_LONG, N, H, seed=7)
    return _CASES[cls]


@pytest.mark.parametrize("gemm", [False, True], ids=["fused", "gemm"])
@pytest.mark.parametrize("reverse", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("cls", lr.CLASSES)
def test_bound_admits_a_correct_kernel(cls, reverse, gemm):
    """The condition on the bound: not one element of a correct float32 kernel over it, in either accumulation order."""
    case = _case(cls)
    for order in (0, 1):
        got = emulate(case, reverse, order, gemm)
        ratio, where = _ratio(case, reverse, got, gemm)
        print("%s %s %s order %d: worst err / bound %.3f at (t, n, unit) = %s" % (cls, "rev" if reverse else "fwd", "gemm" if gemm else "fused", order, ratio, where))
        assert ratio <= 1.0, (cls, reverse, gemm, order, ratio, where)
        if cls == "zeros":
            assert (got.view(torch.int16) == 0).all()
        # sanity at the old tolerance: the free-running fp64 recurrence (typical data; the other classes are not contractive enough to compare trajectories)
        if cls == "typical":
            free = lr.free_running(*case, reverse)
            assert (got.double() - free).abs().max() < 6e-3


# defect -> (data class on which it must show, gemm variant?)
PLANTED = {
    "stale_h": ("typical", False),          # 1  one hidden slice reads h_{t-2} at a single step
    "drop_h_slice": ("typical", False),     # 2  a 32-wide K-slice of the recurrent product dropped
    "drop_x_slice": ("typical", False),     # 3  a 32-wide K-slice of the input product dropped
    "no_bias_gate": ("long_memory", False),  # 4  bias missing on one gate (f)
    "swap_if": ("saturating", False),       # 5  gates i and f swapped for one 8-unit tile
    "c_reset": ("long_memory", False),      # 6  c reset at step 4
    "c_neighbour": ("typical", False),      # 7  c of one ring taken from its neighbour ring
    "forwards": ("typical", False),         # 8  a reverse layer runs forwards
    "g_clamp": ("saturating", False),       # 9  g clamp at +-2.5
    "no_clamp": ("overflow", False),        # 10 i/f/o clamp removed: the shared denominator overflows
    "tanh_approx": ("typical", False),      # 11 tanh(c) with 1e-3 absolute error
    "g_twice": ("typical", True),           # 12 G added twice
    "last_step": ("typical", False),        # 13 the last time step is not written
    "column_shift": ("typical", False),     # 14 a batch column shifted by 16
}


@pytest.mark.parametrize("defect", list(PLANTED))
def test_bound_rejects_a_subtly_wrong_kernel(defect):
    cls, gemm = PLANTED[defect]
    case = _case(cls)
    reverse = defect == "forwards"
    got = emulate(case, reverse, 0, gemm, defect)
    ratio, where = _ratio(case, reverse, got, gemm)
    print("%s on %s: worst err / bound %.3g at %s" % (defect, cls, ratio, where))
    assert ratio > 1.0, (defect, cls, ratio)


def test_fourteen_defects():
    assert len(PLANTED) == 14

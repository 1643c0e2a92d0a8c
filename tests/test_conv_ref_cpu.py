"""tests/conv_ref.py is itself under test (no GPU): `want` against F.conv1d in float64 for every option, the packer's rounding against
torch.half, the bound against a float32 emulation of each kernel's accumulation order (zero elements over it, on every data class the
GPU tests use) and against planted defects (each must exceed the bound or trip a guard)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as cr
from conv_ref import Call, lin_for

INF = float("inf")
WORST = {}               # kind -> (worst err / bound of the correct emulation, case): printed by the last test of the file


def _conv1d(c, t):
    """F.conv1d in float64 on the [N][C][L] view, straight from the description of the operation."""
    x = t["x"].double().permute(0, 2, 1)
    w = cr.weights3(c, t["w"]).double()
    b = t["bias"].double() if c.bias else None
    z = F.conv1d(x, w, b, stride=c.stride, padding=c.pad, groups=c.Cin if c.kind == "dw" else 1)
    return cr.act_fn(c.act, z).clamp(c.lo, c.hi).permute(0, 2, 1)


def _agree_cases():
    out = []
    i = 0
    for kind, cin, cout in (("first", 1, 6), ("igemm", 8, 12), ("dw", 8, 8)):
        for K in (1, 2, 5, 9):
            for stride in (1, 2, 3, 6):
                for pad in sorted({0, K // 2, K - 1}):
                    for lout in (1, 7):
                        i += 1
                        if (lout - 1) * stride + K - 2 * pad + i % stride < 1:          # (Lout = 1 under a pad of K - 1 needs K = 1)
                            continue
                        e = dict(act=i % 4, bias=i % 3 != 0, layout=("NTC", "TNC")[i % 2], os_t=cout + (i % 2) * 8) if kind != "dw" else {}
                        if kind != "dw" and i % 5 == 0:
                            e.update(lo=-0.25, hi=0.5)
                        out.append(Call(kind, 1 + 2 * (i % 2), lin_for(lout, K, stride, pad, extra=i % stride), cin, cout, K, stride, pad, **e))
    return out


@pytest.mark.parametrize("c", _agree_cases(), ids=repr)
def test_want_is_conv1d_in_float64(c):
    t = cr.make_inputs(c, "cpu", 1)
    want, bound = cr.reference(c, t["xbuf"], t["w"], t["bias"])
    assert tuple(want.shape) == (c.N, c.Lout, c.Cout)
    np.testing.assert_allclose(want.numpy(), _conv1d(c, t).numpy(), rtol=1e-12, atol=1e-13)
    assert (bound > 0).all() and torch.isfinite(bound).all()
    rows = c.rows()
    assert sorted(rows.reshape(-1).tolist()) == list(range(c.N * c.Lout))
    os_n, os_t = c.abi_strides()
    n, tt = c.N - 1, c.Lout - 1
    assert n * os_n + tt * os_t == int(rows[n, tt]) * c.os_t
    w = c.writable()
    assert int(w.sum()) == c.N * c.Lout * c.Cout and not w[:, c.Cout:].any() and not w[c.N * c.Lout:].any()


def test_out_len_and_ulp():
    assert [cr.conv_out_len(L, K, s, p) for L, K, s, p in ((10, 5, 1, 2), (10, 5, 3, 0), (19, 19, 6, 0), (1600, 19, 6, 9))] == [10, 2, 1, 267]
    v = torch.tensor([0.0, 1e-9, 2.0 ** -14, 0.75, 1.0, 3.5, -1000.0], dtype=torch.float64)
    assert cr.ulp_fp16(v).tolist() == [2.0 ** -24, 2.0 ** -24, 2.0 ** -24, 2.0 ** -11, 2.0 ** -10, 2.0 ** -9, 0.5]


def test_packer_rounds_like_torch_half():
    """bh_conv1d_pack on values that are NOT representable in fp16 (ties, subnormals, values that round up a binade) stores what
    torch.half stores, at column k * Cin + c, zero in every padding row and column: conv_ref.pack restates it."""
    from bonito_amd import _lib
    c = Call("igemm", 1, 40, 24, 20, 5)
    g = torch.Generator().manual_seed(5)
    w = torch.randn(c.Cout, c.Cin, c.K, generator=g) * 0.3
    w.view(-1)[:8] = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -25, 3 * 2.0 ** -25, 2047.5, -65519.9, 1e-9, 0.1])
    assert not torch.equal(w.half().float(), w)
    n = _lib.lib().bh_conv1d_packed_halves(c.Cin, c.Cout, c.K)
    assert n == 32 * 128
    pk = np.full(n, 0x7E5A, np.uint16)
    wn = w.numpy().copy()
    assert _lib.lib().bh_conv1d_pack(wn.ctypes.data_as(C.c_void_p), c.Cin, c.Cout, c.K, pk.ctypes.data_as(C.c_void_p)) == 0
    mine = cr.pack(c, w).view(torch.int16).numpy().view(np.uint16).reshape(-1)
    assert np.array_equal(pk, mine)


# the shape classes of tests/test_gpu_conv.py (capped at sizes the CPU emulation does in well under a second)
S35 = dict(lo=-0.5, hi=3.5)
CLASSES = [
    Call("first", 3, lin_for(257, 5, 1, 2), 1, 16, 5, 1, 2, act=1, **S35), Call("first", 1, lin_for(255, 19, 6, 9), 1, 6, 19, 6, 9, act=2),
    Call("first", 3, lin_for(1, 9, 2, 0), 1, 344, 9, 2, 0), Call("first", 3, lin_for(65, 2, 3, 1), 1, 4, 2, 3, 1, act=3, bias=False, layout="TNC", os_t=8),
    Call("first", 1, lin_for(70, 1, 1, 0), 1, 24, 1, act=1, lo=-0.25, hi=0.5),
    Call("igemm", 3, lin_for(65, 3, 2, 1), 8, 12, 3, 2, 1, act=1, **S35), Call("igemm", 1, lin_for(129, 5, 1, 4), 24, 20, 5, 1, 4, act=2),
    Call("igemm", 3, lin_for(63, 5, 3, 2), 16, 16, 5, 3, 2, act=1, layout="TNC", os_t=24), Call("igemm", 1, lin_for(80, 9, 2, 4), 128, 64, 9, 2, 4, act=3),
    Call("igemm", 3, lin_for(17, 19, 6, 9), 16, 96, 19, 6, 9, act=1, layout="TNC", **S35), Call("igemm", 1, lin_for(15, 37, 1, 0), 8, 96, 37, bias=False),
    Call("igemm", 1, lin_for(9, 2, 1, 1), 64, 68, 2, 1, 1, act=0, lo=-0.25, hi=0.5), Call("igemm", 3, lin_for(70, 3, 1, 1), 8, 12, 3, 1, 1, act=2, layout="TNC"),
    Call("dw", 3, lin_for(65, 33, 1, 16), 72, 72, 33, 1, 16), Call("dw", 3, lin_for(63, 151, 1, 0), 8, 8, 151), Call("dw", 3, lin_for(129, 3, 2, 1), 64, 64, 3, 2, 1),
    Call("dw", 3, lin_for(1, 1, 2, 0), 8, 8, 1, 2, 0),
]


@pytest.mark.parametrize("cls", cr.DATA_CLASSES)
@pytest.mark.parametrize("c", CLASSES, ids=repr)
def test_bound_admits_a_correct_kernel(c, cls):
    """Each kernel's accumulation order in float32, fp32 epilogue, one rounding: ZERO elements over the bound, every guard intact."""
    t = cr.make_inputs(c, "cpu", 7, cls)
    want, _ = cr.reference(c, t["xbuf"], t["w"], t["bias"])
    assert torch.isfinite(want).all() and float(want.abs().max()) < 65504.0         # the class keeps the reference itself inside fp16
    r = cr.verify(c, t, cr.emulate(c, t, c.alloc_out("cpu")))
    assert cr.ok(r) and r["worst"] < 1.0, cr.message(c, r, "correct emulation, class %s" % cls)
    assert r["worst"] > 0.0
    if r["worst"] > WORST.get(c.kind, (0.0, ""))[0]:
        WORST[c.kind] = (r["worst"], "%r class %s" % (c, cls))


PLANTED = [
    ("last_tap", CLASSES[1], "normal"), ("last_tap", CLASSES[9], "normal"), ("last_tap", CLASSES[14], "normal"), ("last_tap", CLASSES[0], "big"),
    ("pad_off", CLASSES[0], "normal"), ("pad_off", CLASSES[7], "normal"), ("pad_off", CLASSES[13], "normal"),
    ("stride_tap", CLASSES[1], "normal"), ("stride_tap", CLASSES[5], "normal"), ("stride_tap", CLASSES[15], "normal"),
    ("pack_ck", CLASSES[5], "normal"), ("pack_ck", CLASSES[9], "normal"),
    ("kpad_weight", CLASSES[5], "normal"), ("kpad_weight", CLASSES[6], "normal"),
    ("no_bias", CLASSES[0], "normal"), ("no_bias", CLASSES[8], "normal"), ("no_bias", CLASSES[9], "tiny"),
    ("act_swap", CLASSES[0], "normal"), ("act_swap", CLASSES[6], "normal"), ("act_swap", CLASSES[8], "normal"), ("act_swap", CLASSES[2], "normal"),
    ("no_clamp", CLASSES[0], "big"), ("no_clamp", CLASSES[9], "big"), ("no_clamp", CLASSES[11], "normal"), ("no_clamp", CLASSES[4], "normal"),
    ("last_block", CLASSES[0], "normal"), ("last_block", CLASSES[7], "normal"), ("last_block", CLASSES[13], "normal"),
    ("one_past", CLASSES[0], "normal"), ("one_past", CLASSES[7], "normal"), ("one_past", CLASSES[6], "normal"),
    ("layout_swap", CLASSES[3], "normal"), ("layout_swap", CLASSES[5], "normal"), ("layout_swap", CLASSES[7], "normal"),
    ("next_item", CLASSES[0], "normal"), ("next_item", CLASSES[5], "normal"), ("next_item", CLASSES[13], "normal"),
]


@pytest.mark.parametrize("defect,c,cls", PLANTED, ids=lambda v: v if isinstance(v, str) else repr(v))
def test_bound_rejects_a_subtly_wrong_kernel(defect, c, cls):
    """One id per planted defect and kernel kind, on the inputs of the admitted cases. `no_clamp` needs values beyond the clamp: class
    "big" for the model's (-0.5, 3.5), class "normal" for a clamp inside (-1, 1)."""
    t = cr.make_inputs(c, "cpu", 7, cls)
    r = cr.verify(c, t, cr.emulate(c, t, c.alloc_out("cpu"), defect=defect))
    assert not cr.ok(r), "the planted defect %s passed: %s" % (defect, cr.message(c, r))
    if defect == "last_block":
        assert r["lost"] > 0 and r["clobbered"] == 0
    if defect == "one_past":
        assert r["clobbered"] > 0                                   # the last item's extra row lands in the slack rows
    print("%s: %s" % (defect, cr.message(c, r)))


def test_every_defect_is_planted_somewhere():
    assert sorted(set(d for d, _, _ in PLANTED)) == sorted(cr.DEFECTS)
    assert all(any(c is k for k in CLASSES) for _, c, _ in PLANTED)


def test_zz_worst_ratio_of_the_correct_emulation():
    """Not a check of its own: prints the worst err / bound the float32 emulations reached (the figure of DESIGN.md)."""
    for k in sorted(WORST):
        print("%s: worst err / bound %.3f at %s" % (k, WORST[k][0], WORST[k][1]))
    assert all(v[0] < 1.0 for v in WORST.values())

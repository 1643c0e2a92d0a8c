"""The references of tests/quartznet_train_ref.py pinned on the host, and everything about the QuartzNet training layers that needs no
device: the written-out backward of the depthwise convolution, the residual add with activation and dropout and the CTC head against
fp64 autograd and central differences; the fp32 emulation of the device's design within 2 x the fp16 yardstick; planted defects, each
outside that bound; the keep function in Python integers; every refusal of the three train_ops layers and of
bonito_amd.ctc.Model.forward_train; header == binding == exports for the new entry points."""
import math
import os
import re

import pytest
import torch

import conftest
import quartznet_train_ref as ref
from bonito_amd import _lib, train_ops
from bonito_amd.nn import NoTorchCompute

F64 = torch.float64
NEW = ("bh_dwconv1d_train_workspace", "bh_dwconv1d_train_backward", "bh_residual_act_train_forward", "bh_residual_act_train_backward",
       "bh_ctc_head_train_workspace", "bh_ctc_head_train_backward")
# (N, L, C, K, pad): L < K, tails in time and channels, a halo wider than the unit, even K, no padding
DW_CASES = [(1, 5, 8, 9, 4), (3, 65, 16, 33, 16), (2, 130, 8, 123, 61), (2, 70, 16, 4, 2), (2, 9, 8, 3, 0)]
HEAD_CASES = [(1, 8, 2), (257, 40, 5), (130, 16, 8)]
SEED, STREAM = 0x1234567890ABCDEF, 3


def _close(a, b, tol):
    return ref.dist(a, b) <= tol


# ---- formulas == autograd == central differences -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", DW_CASES)
def test_depthwise_formulas_are_fp64_autograd(shape):
    case = ref.dw_case(*shape)
    f, e = ref.dw_formulas(case), ref.dw_exact(case)
    for name in ("y", "dx", "dw"):
        assert f[name].shape == e[name].shape and _close(f[name], e[name], 1e-13), name


def _central(fn, t, idx, h=1e-6):
    old = t[idx].item()
    t[idx] = old + h
    up = fn()
    t[idx] = old - h
    down = fn()
    t[idx] = old
    return (up - down) / (2 * h)


def test_depthwise_formulas_are_central_differences():
    case = {k: (v.to(F64) if isinstance(v, torch.Tensor) else v) for k, v in ref.dw_case(2, 7, 8, 4, 2).items()}
    f = ref.dw_formulas(case)
    loss = lambda: float((ref.dw_formulas(case)["y"] * case["dy"]).sum())      # noqa: E731
    for idx in [(0, 0, 0), (1, 6, 7), (0, 3, 2)]:
        assert abs(_central(loss, case["x"], idx) - float(f["dx"][idx])) < 1e-7
    for idx in [(0, 0, 0), (7, 0, 3), (3, 0, 1)]:
        assert abs(_central(loss, case["w"], idx) - float(f["dw"][idx])) < 1e-7


@pytest.mark.parametrize("shape", HEAD_CASES)
def test_head_formulas_are_fp64_autograd(shape):
    case = ref.head_case(*shape)
    f, e = ref.head_formulas(case), ref.head_exact(case)
    for name in ("lp", "dx", "dw", "db"):
        assert f[name].shape == e[name].shape and _close(f[name], e[name], 1e-12), name


def test_head_formulas_are_central_differences():
    case = {k: v.to(F64) for k, v in ref.head_case(5, 8, 3).items()}
    f = ref.head_formulas(case)
    loss = lambda: float((ref.head_formulas(case)["lp"] * case["dlp"]).sum())      # noqa: E731
    for name, key, idx in [("dx", "x", (4, 7)), ("dx", "x", (0, 0)), ("dw", "w", (2, 3)), ("db", "b", (1,))]:
        assert abs(_central(loss, case[key], idx) - float(f[name][idx])) < 1e-7, name


@pytest.mark.parametrize("act", ref.ACTS)
@pytest.mark.parametrize("with_b", [False, True])
def test_residual_formulas_are_fp64_autograd_and_central_differences(act, with_b):
    case = ref.res_case(13, 8, with_b)
    p = 0.5
    mask = ref.res_mask(case, p, SEED, STREAM)
    f, e = ref.res_formulas(case, act, p, mask), ref.res_exact(case, act, p, mask)
    assert _close(f["y"], e["y"], 1e-14) and _close(f["da"], e["da"], 1e-14)
    c64 = {k: (None if v is None else v.to(F64)) for k, v in case.items()}
    loss = lambda: float((ref.res_formulas(c64, act, p, mask)["y"] * c64["dy"]).sum())      # noqa: E731
    for idx in [(0, 0), (12, 7), (5, 3)]:
        if act == "relu" and abs(float(c64["a"][idx] + (c64["b"][idx] if with_b else 0))) < 1e-3:
            continue
        want = float(f["da"][idx])
        assert abs(_central(loss, c64["a"], idx) - want) < 1e-6
        if with_b:
            assert abs(_central(loss, c64["b"], idx) - want) < 1e-6


# ---- the emulation of the device's design within the bound, planted defects outside -------------------------------------------------------------
@pytest.mark.parametrize("shape", DW_CASES)
def test_depthwise_emulation_is_within_the_bound(shape, capsys):
    case = ref.dw_case(*shape)
    with capsys.disabled():
        bad = ref.within(ref.dw_emulate(case), ref.dw_exact(case), ref.dw_yardstick(case), ("y", "dx", "dw"), "dw %s" % (shape,),
                         say=lambda s: None)
    assert not bad


@pytest.mark.parametrize("defect,shape,name", [("taps_not_flipped", (3, 65, 16, 33, 16), "dx"), ("pad_for_K_1_pad", (2, 70, 16, 4, 2), "dx"),
                                               ("pad_for_K_1_pad", (2, 9, 8, 3, 0), "dx"), ("halo_dropped", (2, 130, 8, 123, 61), "dx"),
                                               ("halo_dropped", (2, 130, 8, 123, 61), "dw"), ("halo_dropped", (3, 65, 16, 33, 16), "dw"),
                                               ("dw_first_item_only", (3, 65, 16, 33, 16), "dw")])
def test_depthwise_defects_are_outside_the_bound(defect, shape, name):
    assert defect in ref.DW_DEFECTS
    case = ref.dw_case(*shape)
    exact, yard = ref.dw_exact(case), ref.dw_yardstick(case)
    assert ref.dist(ref.dw_emulate(case, defect)[name], exact[name]) > 10 * ref.MARGIN * ref.dist(yard[name], exact[name])
    assert not ref.within(ref.dw_emulate(case), exact, yard, (name,), say=lambda s: None)


@pytest.mark.parametrize("shape", HEAD_CASES + [(600, 384, 5)])
def test_head_emulation_is_within_the_bound(shape):
    case = ref.head_case(*shape)
    assert not ref.within(ref.head_emulate(case), ref.head_exact(case), ref.head_yardstick(case), ("lp", "dx", "dw", "db"), say=lambda s: None)


@pytest.mark.parametrize("defect", ref.HEAD_DEFECTS)
def test_head_defects_are_outside_the_bound(defect):
    case = ref.head_case(257, 40, 5)
    exact, yard = ref.head_exact(case), ref.head_yardstick(case)
    got = ref.head_emulate(case, defect)
    for name in ("dx", "dw", "db"):
        assert ref.dist(got[name], exact[name]) > 10 * ref.MARGIN * ref.dist(yard[name], exact[name]), name


@pytest.mark.parametrize("act", ref.ACTS)
@pytest.mark.parametrize("p", [0.0, 0.05, 0.5])
@pytest.mark.parametrize("with_b", [False, True])
def test_residual_emulation_is_within_the_bound(act, p, with_b):
    case = ref.res_case(3 * 65, 72, with_b)
    mask = ref.res_mask(case, p, SEED, STREAM)
    assert bool(mask.all()) == (p == 0.0)
    got = ref.res_emulate(case, act, p, SEED, STREAM)
    assert not ref.within(got, ref.res_exact(case, act, p, mask), ref.res_yardstick(case, act, p, mask), ("y", "da"), say=lambda s: None)
    if p == 0.0:          # the bytes of fp16(act(a + b))
        u = case["a"].float() + (case["b"].float() if with_b else 0.0)
        assert torch.equal(got["y"], ref.act_fn(u, act).half())


@pytest.mark.parametrize("defect", ref.RES_DEFECTS)
def test_residual_defects_are_outside_the_bound(defect):
    case, act, p = ref.res_case(3 * 65, 72, True), "swish", 0.5
    mask = ref.res_mask(case, p, SEED, STREAM)
    exact, yard = ref.res_exact(case, act, p, mask), ref.res_yardstick(case, act, p, mask)
    assert ref.dist(ref.res_emulate(case, act, p, SEED, STREAM, defect)["da"], exact["da"]) > 10 * ref.MARGIN * ref.dist(yard["da"], exact["da"])


# ---- the keep function ----------------------------------------------------------------------------------------------------------------------------
def test_keep_function_in_python_integers():
    # splitmix64's published first output for state 0 is mix(G): the finaliser is the textbook one
    assert ref.mix(ref.GOLDEN) == 0xE220A8397B1DCDAF
    for seed, sid in [(0, 0), (SEED, STREAM), ((1 << 64) - 1, (1 << 64) - 1)]:
        idx = [0, 1, 7, 1000, (1 << 31) - 1, 1 << 31, (1 << 40) + 5]
        for p in (0.05, 0.5):
            for i in idx:
                assert bool(ref.keep_mask(seed, sid, 1, p, start=i)[0]) == ref.keep(seed, sid, i, p)
        assert all(0 <= ref.keep_bits(seed, sid, i) < 1 << 32 for i in idx)


@pytest.mark.parametrize("p", [0.05, 0.5])
def test_kept_fraction_is_binomial(p):
    n = 1 << 20
    kept = int(ref.keep_mask(SEED, STREAM, n, p).sum())
    assert abs(kept - n * (1 - p)) <= 5 * math.sqrt(n * p * (1 - p)), kept


def test_p_zero_keeps_all_and_masks_differ_by_seed_and_stream():
    n = 1 << 16
    assert bool(ref.keep_mask(SEED, STREAM, n, 0.0).all())
    base = ref.keep_mask(SEED, STREAM, n, 0.5)
    for other in (ref.keep_mask(SEED + 1, STREAM, n, 0.5), ref.keep_mask(SEED, STREAM + 1, n, 0.5)):
        assert abs(int((base != other).sum()) - n / 2) <= 5 * math.sqrt(n / 4)
    assert torch.equal(base, ref.keep_mask(SEED, STREAM, n, 0.5))


def test_p_threshold_at_the_ends_of_the_range():
    assert ref.p_threshold(0.0) == 0 and ref.p_threshold(0.5) == 1 << 31
    assert ref.p_threshold(2.0 ** -33) == 0 and ref.p_threshold(2.0 ** -32) == 1
    assert ref.p_threshold(1.0 - 2.0 ** -53) == (1 << 32) - 1              # the largest double below 1 still fits 32 bits
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            ref.p_threshold(bad)
    for p in (0.0, 0.05, 0.5, 1.0 - 2.0 ** -53):
        thr, inv = train_ops.keep_threshold(p)
        assert thr == ref.p_threshold(p) and inv == 1.0 / (1.0 - p)
    with pytest.raises(ValueError):
        train_ops.keep_threshold(1.0)


# ---- refusals, all in front of any launch (CPU tensors reach NoTorchCompute only when everything else is right) ---------------------------------------
def _raises(fn, text, exc=ValueError):
    with pytest.raises(exc) as e:
        fn()
    assert text in str(e.value), str(e.value)


def test_depthwise_refusals():
    x, w = torch.zeros(2, 9, 8, dtype=torch.float16), torch.zeros(8, 1, 3)
    dy = torch.zeros(2, 9, 8, dtype=torch.float16)
    for fn in (train_ops.depthwise_conv1d, train_ops.depthwise_conv1d_forward):
        _raises(lambda: fn(x, w, 1), "HIP device only", NoTorchCompute)
        _raises(lambda: fn(x, torch.zeros(8, 2, 3), 1), "[C][1][K]")
        _raises(lambda: fn(x, w.half(), 1), "float32")
        _raises(lambda: fn(x[:, :, :4], torch.zeros(4, 1, 3), 1), "multiple of 8")
        _raises(lambda: fn(x, torch.zeros(8, 1, 128), 64), "K <= 127")
        _raises(lambda: fn(x, w, 3), "padding < K")
        _raises(lambda: fn(x[:, :2], w, 0), "one whole window")
        _raises(lambda: fn(x.double(), w, 1), "x must be")
        _raises(lambda: fn(x[0], w, 1), "[N][L][8]")
        _raises(lambda: fn(None, w, 1), "must be a tensor")
    _raises(lambda: train_ops.depthwise_conv1d_forward(x.float(), w, 1), "x must be float16")
    _raises(lambda: train_ops.depthwise_conv1d_backward(x, w, dy, 1), "HIP device only", NoTorchCompute)
    _raises(lambda: train_ops.depthwise_conv1d_backward(x, w, dy[:, :8], 1), "dy must be float16")
    _raises(lambda: train_ops.depthwise_conv1d_backward(x, w, dy.float(), 1), "dy must be float16")


def test_residual_act_refusals():
    a = torch.zeros(5, 8, dtype=torch.float16)
    for fn in (train_ops.residual_act, train_ops.residual_act_forward):
        _raises(lambda: fn(a, a, "swish", 0.5, 1, 2), "HIP device only", NoTorchCompute)
        _raises(lambda: fn(a, None, "swish", 0.5, 1, 2), "HIP device only", NoTorchCompute)
        _raises(lambda: fn(a, a[:4], "swish", 0.5, 1, 2), "one shape")
        _raises(lambda: fn(a, a, "gelu", 0.5, 1, 2), "activation")
        _raises(lambda: fn(a, a, "swish", 1.0, 1, 2), "0 <= p < 1")
        _raises(lambda: fn(a, a, "swish", -0.1, 1, 2), "0 <= p < 1")
        _raises(lambda: fn(a, a, "swish", 0.5, -1, 2), "2^64")
        _raises(lambda: fn(a, a, "swish", 0.5, 1, 1 << 64), "2^64")
        _raises(lambda: fn(a[:, :4], None, "swish", 0.5, 1, 2), "multiple of 8")
        _raises(lambda: fn(a.double(), None, "swish", 0.5, 1, 2), "a must be")
        _raises(lambda: fn(a[0], None, "swish", 0.5, 1, 2), "[...][C]")
    _raises(lambda: train_ops.residual_act_forward(a.float(), None), "a must be float16")
    _raises(lambda: train_ops.residual_act_backward(a, a, a, "swish", 0.5, 1, 2), "HIP device only", NoTorchCompute)
    _raises(lambda: train_ops.residual_act_backward(a, a, a.float(), "swish", 0.5, 1, 2), "dy must be float16")


def test_ctc_head_refusals():
    x, w, b = torch.zeros(2, 7, 16, dtype=torch.float16), torch.zeros(5, 16, 1), torch.zeros(5)
    for fn in (train_ops.ctc_head, train_ops.ctc_head_forward):
        _raises(lambda: fn(x, w, b), "HIP device only", NoTorchCompute)
        _raises(lambda: fn(x, w[:, :, 0], b), "[classes][F][1]")
        _raises(lambda: fn(x, torch.zeros(9, 16, 1), torch.zeros(9)), "classes <= 8")
        _raises(lambda: fn(x[:, :, :12], torch.zeros(5, 12, 1), b), "F % 8 == 0")
        _raises(lambda: fn(x.repeat(1, 1, 256), torch.zeros(5, 4096, 1), b), "64 KiB")
        _raises(lambda: fn(x, w.half(), b), "float32")
        _raises(lambda: fn(x, w, b[:4]), "bias must be")
        _raises(lambda: fn(x[0], w, b), "[N][T][16]")
        _raises(lambda: fn(x.double(), w, b), "x must be")
    _raises(lambda: train_ops.ctc_head_backward(x, w, b, torch.zeros(2, 7, 5, dtype=torch.float16)), "HIP device only", NoTorchCompute)
    _raises(lambda: train_ops.ctc_head_backward(x, w, b, torch.zeros(2, 7, 8, dtype=torch.float16)), "dlp must be float16")


def _model(cfg=None, **block0):
    from bonito_amd.ctc import Model
    base, sd, x, _ = conftest.load_ctc_fixture()
    if cfg is None and not block0:
        model = Model(base)
        model.load_state_dict(sd)
    else:
        cfg = cfg or {**base, "block": [{**b} for b in base["block"]]}
        model = Model(cfg)
    return model.train(), x.half()


def _state(model):
    return {k: v.clone() for k, v in model.state_dict().items()}


def test_forward_train_without_norm_is_refused_with_no_side_effect():
    model, x = _model()
    before, rng = _state(model), torch.get_rng_state()
    _raises(lambda: model.forward_train(x), "has no forward_train")
    _raises(lambda: model.forward_train(x, norm=None), "has no forward_train")
    _raises(lambda: model.forward_train(x, norm="layer"), "norm='layer' is not served")
    after = _state(model)
    assert all(torch.equal(before[k], after[k]) for k in before) and torch.equal(rng, torch.get_rng_state())
    assert model._hip is None


def test_forward_train_refusals_name_the_block_and_change_nothing():
    base = conftest.load_ctc_fixture()[0]

    def cfg(i, **kw):
        return {**base, "block": [{**b, **(kw if j == i else {})} for j, b in enumerate(base["block"])]}

    model, x = _model()
    before, rng = _state(model), torch.get_rng_state()
    _raises(lambda: model.forward_train(x, norm="batch"), "HIP device only", NoTorchCompute)
    _raises(lambda: model.forward_train(x.float(), norm="batch"), "float16 tensor [N,1,L]")
    _raises(lambda: model.forward_train(x[:, 0], norm="batch"), "float16 tensor [N,1,L]")
    model.encoder.encoder[2].conv[1].eval()
    _raises(lambda: model.forward_train(x, norm="batch"), "encoder.encoder.2.conv.0 has its BatchNorm in eval mode")
    model.train()
    model.eval()
    _raises(lambda: model.forward_train(x, norm="batch"), "encoder.encoder.0.conv.0 has its BatchNorm in eval mode")
    model.train()
    model.encoder.encoder[1].conv[0].pointwise.half()
    _raises(lambda: model.forward_train(x, norm="batch"), "encoder.encoder.1.conv.0.pointwise holds torch.float16 parameters")
    model.encoder.encoder[1].conv[0].pointwise.float()
    after = _state(model)
    assert all(torch.equal(before[k], after[k]) for k in before) and torch.equal(rng, torch.get_rng_state())
    for c, text in [(cfg(1, dilation=[2]), "encoder.encoder.1.conv.0.depthwise has dilation 2"),
                    (cfg(4, dilation=[2]), "encoder.encoder.4.conv.0.conv has dilation 2"),
                    (cfg(1, stride=[2]), "encoder.encoder.1.conv.0 is a separable convolution with stride 2"),
                    (cfg(3, kernel=[129]), "encoder.encoder.3.conv.0 is a separable convolution with stride 1 and K = 129"),
                    (cfg(1, filters=44), "encoder.encoder.1.conv.0 has 32 -> 44 channels"),
                    (cfg(0, kernel=[33]), "encoder.encoder.0.conv.0.conv: K <= 32"),       # dna_r9.4.1@v1's first layer: train_ops.conv1d's own message
                    (cfg(0, filters=4104), "encoder.encoder.0.conv.0.conv: shape N=3 Lin=600 Cin=1 Cout=4104"),   # the library's own limit
                    (cfg(2, kernel=[4]), "encoder.encoder.2 adds a residual of 200 steps")]:
        m, _ = _model(c)
        rng = torch.get_rng_state()
        _raises(lambda: m.forward_train(x, norm="batch"), text)
        assert torch.equal(rng, torch.get_rng_state()), "a call that _train_plan refuses draws no seed: %s" % text
    six = {**base, "labels": {"labels": list("NACGTUXYZ")}}
    m, _ = _model(six)
    _raises(lambda: m.forward_train(x, norm="batch"), "decoder: classes <= 8")


# ---- header == binding == exports ---------------------------------------------------------------------------------------------------------------
def test_new_entry_points_are_declared_bound_and_exported():
    text = open(os.path.join(conftest.ROOT, "include", "bonito_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = _lib.lib()
    for name in NEW:
        decl = re.search(r"\b(size_t|int)\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert decl, "%s is not declared in include/bonito_hip.h" % name
        assert name in _lib.SIGNATURES and hasattr(handle, name)
        res, args = _lib.SIGNATURES[name]
        assert len(args) == len(decl.group(2).split(",")), name
        assert (res is _lib._sz) == (decl.group(1) == "size_t"), name
    top = text.split("#ifndef BONITO_HIP_H")[0]
    assert "bh_dwconv1d_train_backward" in top and "bh_ctc_head_train_backward" in top and "bh_residual_act_train_forward" in top
    # an unsupported shape has no workspace: 0, and nothing else is asked of the device
    assert handle.bh_dwconv1d_train_workspace(2, 64, 12, 5, 2) == 0 and handle.bh_dwconv1d_train_workspace(2, 64, 16, 128, 2) == 0
    assert handle.bh_dwconv1d_train_workspace(2, 64, 16, 5, 5) == 0 and handle.bh_dwconv1d_train_workspace(2, 3, 16, 5, 0) == 0
    assert handle.bh_ctc_head_train_workspace(10, 16, 9) == 0 and handle.bh_ctc_head_train_workspace(10, 12, 5) == 0
    assert handle.bh_ctc_head_train_workspace(10, 4096, 5) == 0 and handle.bh_ctc_head_train_workspace(0, 16, 5) == 0
    tiles, per, blocks = ref.dw_blocks(3, 65, 72, 33, 16)
    assert handle.bh_dwconv1d_train_workspace(3, 65, 72, 33, 16) == -(-(blocks * 72 * 33 * 4) // 256) * 256

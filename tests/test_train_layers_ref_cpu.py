"""The references of the training convolution / linear layer (tests/train_layers_ref.py) pinned on the CPU, the margin of the device
tests justified by an emulation of the device's design, the planted defects, and every refusal of bonito_amd.train_ops and
SeqdistModel.forward_train that needs no device."""
import functools
import re

import pytest
import torch

import train_layers_ref as tl
from conftest import ROOT

CONV_VARIANTS = [(case, clamp, scale) for case in tl.CONV_CASES for clamp in (None, tl.CLAMP) for scale in (1.0, 4.0)]


def _conv_id(v):
    case, clamp, scale = v
    return "%s-%s-x%g" % ("x".join(str(c) for c in case), "clamp" if clamp else "free", scale)


@functools.lru_cache(maxsize=None)
def _conv_refs(case, clamp, scale):
    x, w, b, dy, pad = tl.conv_inputs(case, scale)
    stride = case[4]
    y16, m, emu = tl.conv_emulate(x, w, b, dy, stride, pad, "swish", clamp)
    return (x, w, b, dy, pad, m), tl.conv_exact(x, w, b, m, dy, stride, pad, "swish"), tl.conv_yardstick(x, w, b, m, dy, stride, pad, "swish"), emu


@functools.lru_cache(maxsize=None)
def _linear_refs(case):
    T, N, K, C, act, scale, clamp, bias = case
    x, w, b, dy = tl.linear_inputs(case)
    y16, m, emu = tl.linear_emulate(x, w, b, dy, act, scale, clamp)
    return (x, w, b, dy, m), tl.linear_exact(x, w, b, m, dy, act, scale), tl.linear_yardstick(x, w, b, m, dy, act, scale), emu


# ---- the references themselves -----------------------------------------------------------------------------------------------------------
def _finite_difference(f, leaves, dy, eps=1e-6):
    grads = []
    for t in leaves:
        g = torch.zeros_like(t)
        flat, gf = t.view(-1), g.view(-1)
        for i in range(flat.numel()):
            old = float(flat[i])
            flat[i] = old + eps
            up = float((f() * dy).sum())
            flat[i] = old - eps
            dn = float((f() * dy).sum())
            flat[i] = old
            gf[i] = (up - dn) / (2 * eps)
        grads.append(g)
    return grads


def test_exact_convolution_agrees_with_central_finite_differences():
    g = torch.Generator().manual_seed(1)
    N, Cin, Cout, K, stride, Lin, pad = 2, 3, 4, 5, 2, 12, 2
    x, w, b = torch.randn(N, Lin, Cin, generator=g).half(), torch.randn(Cout, Cin, K, generator=g).half().float(), torch.randn(Cout, generator=g).half().float()
    Lout = tl.conv_out_len(Lin, K, stride, pad)
    dy = torch.randn(N, Lout, Cout, generator=g).half()
    m = torch.rand(N, Lout, Cout, generator=g) > 0.3
    got = tl.conv_exact(x, w, b, m, dy, stride, pad, "swish")
    xd, wd, bd = x.double(), w.double(), b.double()
    f = lambda: torch.nn.functional.silu(torch.nn.functional.conv1d(xd.permute(0, 2, 1), wd, bd, stride=stride, padding=pad)).permute(0, 2, 1) * m   # noqa: E731
    for name, fd in zip(("dx", "dw", "db"), _finite_difference(f, [xd, wd, bd], dy.double())):
        assert tl.dist(got[name], fd) < 1e-7, name


def test_exact_linear_agrees_with_central_finite_differences():
    g = torch.Generator().manual_seed(2)
    T, N, K, C = 3, 2, 8, 8
    x, w, b = torch.randn(T, N, K, generator=g).half(), torch.randn(C, K, generator=g).half().float() / 2, torch.randn(C, generator=g).half().float()
    dy = torch.randn(T, N, C, generator=g).half()
    m = torch.rand(T, N, C, generator=g) > 0.3
    got = tl.linear_exact(x, w, b, m, dy, "tanh", 5.0)
    xd, wd, bd = x.double(), w.double(), b.double()
    f = lambda: torch.tanh(torch.nn.functional.linear(xd, wd, bd)) * 5.0 * m      # noqa: E731
    for name, fd in zip(("dx", "dw", "db"), _finite_difference(f, [xd, wd, bd], dy.double())):
        assert tl.dist(got[name], fd) < 1e-7, name


def test_emulation_forward_is_the_convolution():
    x, w, b, dy, pad = tl.conv_inputs(tl.CONV_CASES[4])
    y16, m, _ = tl.conv_emulate(x, w, b, dy, 5, pad, "swish", tl.CLAMP)
    want = torch.nn.functional.silu(torch.nn.functional.conv1d(x.double().permute(0, 2, 1), w.half().double(), b.half().double(), stride=5, padding=pad))
    assert tl.dist(y16, want.clamp(*tl.CLAMP).permute(0, 2, 1)) < 1e-3
    assert 0 < int(m.sum()) < m.numel()


# ---- the margin: the design itself, in fp32 on the CPU, against the yardstick ------------------------------------------------------------
@pytest.mark.parametrize("variant", CONV_VARIANTS, ids=_conv_id)
def test_convolution_emulation_is_within_twice_the_yardstick(variant):
    _, exact, yard, emu = _conv_refs(*variant)
    for name in ("dx", "dw", "db"):
        d, dy = tl.dist(emu[name], exact[name]), tl.dist(yard[name], exact[name])
        print("conv %s %s: emulation %.3e yardstick %.3e ratio %.2f" % (_conv_id(variant), name, d, dy, d / dy))
        assert d <= tl.MARGIN * dy, name


@pytest.mark.parametrize("case", tl.LINEAR_CASES, ids=lambda c: "x".join(str(v) for v in c[:4]))
def test_linear_emulation_is_within_twice_the_yardstick(case):
    _, exact, yard, emu = _linear_refs(case)
    for name in ("dx", "dw", "db"):
        if exact[name] is None:
            continue
        d, dy = tl.dist(emu[name], exact[name]), tl.dist(yard[name], exact[name])
        print("linear %s %s: emulation %.3e yardstick %.3e ratio %.2f" % (case[:4], name, d, dy, d / dy))
        assert d <= tl.MARGIN * dy, name


# ---- planted defects fall outside the margin, on the device tests' own inputs ------------------------------------------------------------
_BREAKS = {"tap_off_by_one": "dw", "stride_on_tap": "dw", "padding_off_by_one": "dw", "mask_inclusive": "dw", "last_row_block_dropped": "dw",
           "bias_wrong_axis": "db", "scale_omitted": "dw", "dx_through_w": "dx"}


# (stride 1: the tap and the position have the same stride, the defect changes nothing)
@pytest.mark.parametrize("case,defect", [(c, d) for c in tl.CONV_CASES for d in tl.CONV_DEFECTS if not (d == "stride_on_tap" and c[4] == 1)],
                         ids=lambda v: v if isinstance(v, str) else "x".join(str(c) for c in v))
def test_planted_convolution_defects_fall_outside_the_margin(case, defect):
    # (the inclusive mask shows where outputs sit ON a bound: input scale 4 has them in every case)
    (x, w, b, dy, pad, m), exact, yard, _ = _conv_refs(case, tl.CLAMP, 4.0 if defect == "mask_inclusive" else 1.0)
    _, _, bad = tl.conv_emulate(x, w, b, dy, case[4], pad, "swish", tl.CLAMP, defect=defect)
    name = _BREAKS[defect]
    assert tl.dist(bad[name], exact[name]) > tl.MARGIN * tl.dist(yard[name], exact[name]), (defect, name)
    if defect in ("tap_off_by_one", "stride_on_tap", "padding_off_by_one", "mask_inclusive"):
        assert tl.dist(bad["dx"], exact["dx"]) > tl.MARGIN * tl.dist(yard["dx"], exact["dx"]), (defect, "dx")


def _linear_defect_applies(case, defect):
    T, N, K, C, act, scale, clamp, bias = case
    return not ((defect == "scale_omitted" and scale is None) or (defect == "mask_inclusive" and clamp is None)
                or (defect == "bias_wrong_axis" and not bias))


@pytest.mark.parametrize("case,defect", [(c, d) for c in tl.LINEAR_CASES for d in tl.LINEAR_DEFECTS if _linear_defect_applies(c, d)],
                         ids=lambda v: v if isinstance(v, str) else "x".join(str(c) for c in v[:4]))
def test_planted_linear_defects_fall_outside_the_margin(case, defect):
    T, N, K, C, act, scale, clamp, bias = case
    (x, w, b, dy, m), exact, yard, _ = _linear_refs(case)
    _, _, bad = tl.linear_emulate(x, w, b, dy, act, scale, clamp, defect=defect)
    name = _BREAKS[defect]
    assert tl.dist(bad[name], exact[name]) > tl.MARGIN * tl.dist(yard[name], exact[name]), (defect, name)


def test_the_clamped_cases_have_elements_on_a_bound():
    for case in tl.CONV_CASES:
        x, w, b, dy, pad = tl.conv_inputs(case, 4.0)
        y16, m, _ = tl.conv_emulate(x, w, b, dy, case[4], pad, "swish", tl.CLAMP)
        assert int((y16.float() == tl.CLAMP[1]).sum()) > 0 and not bool(m[y16.float() == tl.CLAMP[1]].any())
    case = tl.LINEAR_CASES[3]
    x, w, b, dy = tl.linear_inputs(case)
    y16, m, _ = tl.linear_emulate(x, w, b, dy, case[4], case[5], case[6])
    assert int((y16.float().abs() == 5.0).sum()) > 0 and int(m.sum()) > 0


# ---- the chain of tests/test_gpu_train_model.py ---------------------------------------------------------------------------------------
CHAIN = dict(features=32, first_conv=4, stride=5, winlen=19, n_layers=5, n_out=256)      # state_len 3, blank_score 2.0: 4^4 outputs


def test_chain_emulation_against_the_yardstick():
    """The whole chain conv x3 -> LSTM x5 -> tanh head with every activation and gradient stored as fp16 (fp32 arithmetic), against the
    same chain in fp16 on the CPU, both against fp64: the ratios decide the margin of the device test (2, unless the emulation alone
    passes 1.5 on a parameter)."""
    g = torch.Generator().manual_seed(77)
    signal = torch.randn(3, 120, generator=g).half()
    params = tl.chain_params(**CHAIN)
    dscores = (torch.randn(3, 24, 256, generator=g) * 0.05).half()
    kw = dict(stride=5, n_layers=5, scale=5.0)
    y64, exact = tl.chain_ref(signal, params, dscores, dtype=torch.float64, **kw)
    y16, yard = tl.chain_ref(signal, params, dscores, dtype=torch.float16, **kw)
    y32, emu = tl.chain_ref(signal, params, dscores, dtype=torch.float32, emulate=True, **kw)
    assert y64.shape == (3, 24, 256) and tl.dist(y16, y64) < 5e-3 and tl.dist(y32, y64) < 5e-3
    for name, _ in params:
        d, dy = tl.dist(emu[name], exact[name]), tl.dist(yard[name], exact[name])
        print("chain %s: emulation %.3e yardstick %.3e ratio %.2f" % (name, d, dy, d / dy))
        assert d <= 1.5 * dy, name


# ---- refusals that need no device --------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported():
    from bonito_amd import _lib
    names = ["bh_conv1d_train_workspace", "bh_conv1d_train_forward", "bh_conv1d_train_backward", "bh_linear_train_workspace",
             "bh_linear_train_forward", "bh_linear_train_backward"]
    header = re.sub(r"/\*.*?\*/", "", open(ROOT + "/include/bonito_hip.h").read(), flags=re.S)
    handle = _lib.lib()
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, header) and n in _lib.SIGNATURES and hasattr(handle, n), n


def test_workspace_sizes_refuse_unsupported_shapes():
    from bonito_amd import _lib
    lib = _lib.lib()
    assert lib.bh_conv1d_train_workspace(3, 403, 16, 96, 19, 5, 9) > 0 and lib.bh_conv1d_train_workspace(3, 203, 1, 4, 5, 1, 2) > 0
    for bad in ((3, 403, 4, 96, 19, 5, 9), (3, 403, 16, 98, 19, 5, 9), (3, 403, 16, 96, 33, 5, 9), (3, 403, 16, 96, 19, 9, 9),
                (3, 403, 16, 96, 19, 5, 19), (3, 10, 16, 96, 19, 5, 2), (0, 403, 16, 96, 19, 5, 9)):
        assert lib.bh_conv1d_train_workspace(*bad) == 0, bad
    assert lib.bh_linear_train_workspace(20, 3, 96, 1024) > 0
    for bad in ((20, 3, 100, 1024), (20, 3, 96, 1020), (0, 3, 96, 1024), (20, 0, 96, 1024)):
        assert lib.bh_linear_train_workspace(*bad) == 0, bad


def test_buffer_sizes_equal_the_parent_commit():
    """tests/golden/train_parent.json was written by tests/golden/make_golden_train_parent.py at the commit it names, before the
    layers shared one reduction over rows. The partial sums of the weight gradients are the tail of every workspace, so equal sizes
    mean equal block counts: the order of the sums. The table holds every CONV_CASES and LINEAR_CASES row, and for the LSTM layer
    shapes where the cap on the blocks binds (H = 1024) and where the last block is short (150 x 20 at H = 64)."""
    import json
    from bonito_amd import _lib
    with open(ROOT + "/tests/golden/train_parent.json") as fh:
        gold = json.load(fh)
    lib = _lib.lib()
    assert len(gold["lstm"]) == 6 * 5 and len(gold["linear"]) == len(tl.LINEAR_CASES)
    assert {(r[0], r[2], r[3], r[4], r[5], r[1]) for r in gold["conv"]} >= set(tl.CONV_CASES)
    assert [64, 150, 20] in [[r[2], r[0], r[1]] for r in gold["lstm"]] and [1024, 600, 64] in [[r[2], r[0], r[1]] for r in gold["lstm"]]
    for T, N, H, saved, work in gold["lstm"]:
        assert lib.bh_lstm_train_saved_bytes(T, N, H) == saved and lib.bh_lstm_train_backward_workspace(T, N, H) == work, (T, N, H)
    for *shape, want in gold["conv"]:
        assert lib.bh_conv1d_train_workspace(*shape) == want, shape
    for *shape, want in gold["linear"]:
        assert lib.bh_linear_train_workspace(*shape) == want, shape


def test_entry_points_refuse_before_any_device_call():
    """The argument checks stand in front of every launch: the pointers below are never read."""
    import ctypes as C
    from bonito_amd import _lib
    lib, p = _lib.lib(), C.c_void_p(4096)
    rc = lib.bh_conv1d_train_forward(p, p, p, 3, 403, 12, 96, 19, 5, 9, 1, -0.5, 3.5, 96, 3 * 96, p, p, 1 << 30, None)
    assert rc != 0 and "Cin must be 1 or a multiple of 8" in _lib.last_error()
    rc = lib.bh_conv1d_train_backward(p, p, p, p, p, 3, 403, 16, 96, 19, 5, 9, 1, -0.5, 3.5, 96, 3 * 96, p, p, p, p, 16, None)
    assert rc != 0 and "workspace of 16 bytes" in _lib.last_error()
    rc = lib.bh_conv1d_train_backward(p, p, p, None, p, 3, 403, 16, 96, 19, 5, 9, 1, -0.5, 3.5, 96, 3 * 96, p, p, p, p, 1 << 30, None)
    assert rc != 0 and "null pointer" in _lib.last_error()
    rc = lib.bh_linear_train_forward(p, p, p, 20, 3, 96, 1024, 1, 5.0, -5.0, 5.0, 1, p, p, 1 << 30, None)
    assert rc != 0 and "activation 1 is not supported" in _lib.last_error()
    rc = lib.bh_linear_train_backward(p, p, p, p, 20, 3, 96, 1020, 2, 5.0, -5.0, 5.0, 1, p, p, p, p, 1 << 30, None)
    assert rc != 0 and "C must be a multiple of 8" in _lib.last_error()
    rc = lib.bh_linear_train_backward(p, p, p, p, 20, 3, 96, 1024, 2, 0.0, -5.0, 5.0, 1, p, p, p, p, 1 << 30, None)
    assert rc != 0 and "scale must be finite and not 0" in _lib.last_error()


def test_wrappers_refuse_host_tensors_and_wrong_arguments():
    from bonito_amd import train_ops
    from bonito_amd.nn import NoTorchCompute
    x, w, b = torch.zeros(2, 50, 16, dtype=torch.float16), torch.zeros(32, 16, 5), torch.zeros(32)
    with pytest.raises(NoTorchCompute):
        train_ops.conv1d_forward(x, w, b, 1, 2, "swish")
    with pytest.raises(NoTorchCompute):
        train_ops.conv1d(x.float().requires_grad_(), w, b, 1, 2, "swish")
    with pytest.raises(NoTorchCompute):
        train_ops.conv1d(torch.zeros(2, 50, 4, dtype=torch.float16), torch.zeros(32, 4, 5), b, 1, 2, "swish")
    with pytest.raises(NoTorchCompute):
        train_ops.conv1d_backward(x, w, b, torch.zeros(2, 50, 32, dtype=torch.float16), torch.zeros(2, 50, 32, dtype=torch.float16), 1, 2, "swish")
    for kw, text in ((dict(x=x.float()), "x must be float16"), (dict(w=w.half()), "must be float32"), (dict(w=torch.zeros(32, 12, 5)), "x must be"),
                     (dict(b=torch.zeros(31)), "bias must be"), (dict(stride=9), "stride <= 8"), (dict(padding=5), "padding < K"),
                     (dict(activation="gelu"), "activation"), (dict(clamp=(1.0, -1.0)), "empty"), (dict(w=torch.zeros(30, 16, 5), b=None), "Cout a multiple of 4"),
                     (dict(x=torch.zeros(2, 50, dtype=torch.float16)), "x must be")):
        a = dict(x=x, w=w, b=b, stride=1, padding=2, activation="swish", clamp=None)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            train_ops.conv1d_forward(a["x"], a["w"], a["b"], a["stride"], a["padding"], a["activation"], a["clamp"])
    with pytest.raises(ValueError, match="dy must be float16"):
        train_ops.conv1d_backward(x, w, b, torch.zeros(2, 50, 32, dtype=torch.float16), torch.zeros(2, 49, 32, dtype=torch.float16), 1, 2, "swish")
    X, W, B = torch.zeros(7, 3, 64, dtype=torch.float16), torch.zeros(256, 64), torch.zeros(256)
    with pytest.raises(NoTorchCompute):
        train_ops.linear_forward(X, W, B, "tanh", 5.0)
    with pytest.raises(NoTorchCompute):
        train_ops.linear(X.float(), W, B, "tanh", 5.0)
    with pytest.raises(NoTorchCompute):
        train_ops.linear_backward(X, W, torch.zeros(7, 3, 256, dtype=torch.float16), torch.zeros(7, 3, 256, dtype=torch.float16), "tanh", 5.0)
    for kw, text in ((dict(x=X.float()), "x must be float16"), (dict(w=W.half()), "must be float32"), (dict(w=torch.zeros(256, 60)), "x must be"),
                     (dict(w=torch.zeros(250, 64), b=None), "multiples of 8"), (dict(b=torch.zeros(255)), "bias must be"),
                     (dict(activation="swish"), "activation"), (dict(scale=0.0), "scale must be"), (dict(clamp=(5.0, -5.0)), "empty")):
        a = dict(x=X, w=W, b=B, activation="tanh", scale=5.0, clamp=None)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            train_ops.linear_forward(a["x"], a["w"], a["b"], a["activation"], a["scale"], a["clamp"])
    with pytest.raises(ValueError, match="y must be float16"):
        train_ops.linear_backward(X, W, torch.zeros(3, 7, 256, dtype=torch.float16), torch.zeros(7, 3, 256, dtype=torch.float16), "tanh", 5.0)


def _config(norm=None, kind="lstm"):
    conv = lambda i, o, k, s=1: dict(type="convolution", insize=i, size=o, winlen=k, stride=s, padding=k // 2, bias=True, activation="swish",   # noqa: E731
                                     **({"norm": norm} if norm else {}))
    clamp = dict(type="clamp", min=-0.5, max=3.5)
    body = [dict(type="lstm", size=32, insize=32, bias=True, reverse=bool(i % 2 == 0)) for i in range(2)]
    if kind == "upsample":
        body.append(dict(type="linearupsample", d_model=32, scale_factor=2))
    sub = [conv(1, 4, 5), clamp, conv(4, 16, 5), clamp, conv(16, 32, 19, 5), clamp, dict(type="permute", dims=[2, 0, 1])] + body + [
        dict(type="linear", in_features=32, out_features=64, bias=True),
        dict(type="linearcrfencoder", insize=64, n_base=4, state_len=3, bias=False, scale=5.0, blank_score=2.0, expand_blanks=True),
        dict(type="clamp", min=-5.0, max=5.0)]
    return {"labels": {"labels": ["N", "A", "C", "G", "T"]}, "global_norm": {"state_len": 3}, "input": {"features": 1},
            "encoder": {"type": "serial", "sublayers": sub}}


def _old_config(**enc):
    return {"labels": {"labels": ["N", "A", "C", "G", "T"]}, "global_norm": {"state_len": 3}, "input": {"features": 1},
            "encoder": dict(dict(features=32, stride=5, winlen=19, scale=5.0, blank_score=2.0, num_layers=2, first_conv_size=4), **enc)}


def test_forward_train_refusals_name_the_layer_and_build_no_engine():
    from bonito_amd.crf.model import Model
    from bonito_amd.nn import NoTorchCompute
    x = torch.zeros(2, 1, 120, dtype=torch.float16)
    for model, text in ((Model(_config(norm="batchnorm")), r"layer 0 \(Convolution\) carries a norm \(batchnorm\)"),
                        (Model(_old_config(norm="batchnorm")), r"layer 0 \(Convolution\) carries a norm \(batchnorm\)"),
                        (Model(_config(kind="upsample")), r"layer 9 \(LinearUpsample\) has no training forward"),
                        (Model(_config()).half(), r"layer 0 \(Convolution\) holds float16 parameters"),
                        (Model(_config()).use_hip(quantize=True), "quantize"),
                        (Model(_old_config(features=48)), r"layer 4 \(LSTM\) is not an LSTM the device layer serves")):
        with pytest.raises(ValueError, match=text):
            model.forward_train(x)
        assert model._hip is None
    cfg = _config()
    cfg["encoder"]["sublayers"][1] = dict(type="clamp", min=0.5, max=3.5)       # 4 channels served by zero channels: the range must hold 0
    model = Model(cfg)
    with pytest.raises(ValueError, match=r"layer 0 \(Convolution\) has 4 channels, served by zero padding, and its clamp range"):
        model.forward_train(x)
    assert model._hip is None
    model = Model(_config())
    with pytest.raises(ValueError, match="x must be a float16 tensor"):
        model.forward_train(x.float())
    with pytest.raises(ValueError, match="x must be a float16 tensor"):
        model.forward_train(x[:, 0])
    with pytest.raises(NoTorchCompute):
        model.forward_train(x)
    assert model._hip is None


def test_forward_train_refuses_what_only_the_layout_tells_before_anything_runs():
    """Five encoders whose defect shows in the layout the activations have at a layer: the plan refuses them by name for a CPU x too,
    in front of NoTorchCompute, and the normalised convolution they begin with keeps its statistics and its batch counter."""
    import batchnorm_train_ref as bn
    x = torch.zeros(2, 1, 120, dtype=torch.float16)
    cases = bn.misbuilt_models()
    assert [name for name, _, _ in cases] == ["no head", "lstm without permute", "conv after permute", "stray clamp", "second conv of one channel"]
    for name, model, text in cases:
        before = bn.batchnorm_buffers(model)
        assert sorted(k.rsplit(".", 1)[-1] for k in before) == ["num_batches_tracked", "running_mean", "running_var"], name
        with pytest.raises(ValueError, match=text):
            model.forward_train(x, norm="batch")
        assert model._hip is None, name
        after = bn.batchnorm_buffers(model)
        assert all(torch.equal(before[k], after[k]) for k in before), name


def test_forward_train_refuses_a_transformer_by_name():
    from bonito_amd.crf.model import SeqdistModel, CTC_CRF
    from bonito_amd import nn as bnn

    class TransformerEncoderLayer(torch.nn.Module):
        pass
    enc = bnn.Serial([bnn.Convolution(1, 16, 5, padding=2, activation="swish"), TransformerEncoderLayer(),
                      bnn.LinearCRFEncoder(16, 4, 3, blank_score=2.0)])
    model = SeqdistModel(enc, CTC_CRF(3, ["N", "A", "C", "G", "T"]))
    with pytest.raises(ValueError, match=r"layer 1 \(TransformerEncoderLayer\) has no training forward"):
        model.forward_train(torch.zeros(2, 1, 120, dtype=torch.float16))
    assert model._hip is None

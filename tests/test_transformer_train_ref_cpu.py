"""The references of tests/transformer_train_ref.py pinned on the host, and everything about the transformer family's training layers
that needs no device: the written-out backward of the DeepNorm residual RMSNorm and of fc1 + SwiGLU against fp64 torch autograd and
against central finite differences; the fp32 / fp16-storage emulation of the device's design inside the device tests' margin (2 x the
torch fp16 yardstick) and every planted defect outside it; every refusal of the new train_ops functions, of attn.encoder_layer and of
SeqdistModel.forward_train on CPU tensors; header == binding == exports for the new entry points."""
import os
import re

import pytest
import torch

import transformer_train_ref as ref
from conftest import ROOT

V5_ALPHA = 2.4494897            # deepnorm_params(18)[0]
NORM_SHAPES = ((5, 64), (257, 512), (3, 520), (4, 8), (1, 1024))           # (M, D): shapes of the device test
GATED_SHAPES = ((17, 64, 72), (130, 128, 256), (1, 8, 8))                  # (M, D, F)


# ---- the formulas are the derivative ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", (1.0, V5_ALPHA))
@pytest.mark.parametrize("M,D", ((5, 64), (3, 520)))
def test_norm_formulas_are_fp64_autograd(M, D, alpha):
    case = ref.norm_case(M, D, zero_row=1)
    for name, got, want in zip(ref.NORM_NAMES, ref.norm_formulas(case, alpha), ref.norm_torch(case, alpha)):
        assert ref.dist(got, want) < 1e-12, name


def test_gated_formulas_are_fp64_autograd():
    for M, D, F in GATED_SHAPES:
        case = ref.gated_case(M, D, F)
        for name, got, want in zip(ref.GATED_NAMES, ref.gated_formulas(case), ref.gated_torch(case)):
            assert ref.dist(got, want) < 1e-12, (M, D, F, name)


def _central(f, t, dy, h=1e-6):
    """d <f(t), dy> / dt by central differences, element by element (t float64)."""
    g = torch.zeros_like(t)
    flat, gf = t.view(-1), g.view(-1)
    for i in range(flat.numel()):
        keep = float(flat[i])
        flat[i] = keep + h
        up = float((f() * dy).sum())
        flat[i] = keep - h
        down = float((f() * dy).sum())
        flat[i] = keep
        gf[i] = (up - down) / (2 * h)
    return g


def test_norm_formulas_are_the_central_differences():
    case = ref.norm_case(3, 8, seed=4)
    a, x, w, dy = (case[k].double() for k in ("a", "x", "w", "dy"))
    f = lambda: ref._rms(a + V5_ALPHA * x, w, ref.EPS)      # noqa: E731
    _, da, dx, dw = ref.norm_formulas(case, V5_ALPHA)
    for name, got, t in (("da", da, a), ("dx", dx, x), ("dw", dw, w)):
        assert ref.dist(got, _central(f, t, dy)) < 1e-7, name


def test_gated_formulas_are_the_central_differences():
    case = ref.gated_case(3, 8, 8, seed=4)
    x, w, dh = (case[k].double() for k in ("x", "w", "dh"))

    def f():
        y, gate = (x @ w.T).chunk(2, dim=-1)
        return y * gate * torch.sigmoid(gate)

    _, dx, dw = ref.gated_formulas(case)
    for name, got, t in (("dx", dx, x), ("dw", dw, w)):
        assert ref.dist(got, _central(f, t, dh)) < 1e-7, name


# ---- the emulation inside the margin, the defects outside ------------------------------------------------------------------------------------
def _norm_ratios(case, alpha, defect=None):
    exact, yard = ref.norm_torch(case, alpha), ref.norm_torch(case, alpha, dtype=torch.float16)
    got = ref.norm_formulas(case, alpha, emulate=True, defect=defect)
    return {n: (ref.dist(g, e), ref.dist(y, e)) for n, g, e, y in zip(ref.NORM_NAMES, got, exact, yard)}


@pytest.mark.parametrize("alpha", (1.0, V5_ALPHA))
@pytest.mark.parametrize("M,D", NORM_SHAPES)
def test_norm_emulation_is_inside_the_margin(M, D, alpha):
    for name, (dk, dy) in _norm_ratios(ref.norm_case(M, D), alpha).items():
        print("norm M=%d D=%d alpha=%g %-3s: dist(emulation) = %.3e  dist(yardstick) = %.3e" % (M, D, alpha, name, dk, dy))
        assert dk <= ref.MARGIN * dy, name


@pytest.mark.parametrize("defect", ref.NORM_DEFECTS)
def test_norm_defects_are_outside_the_margin(defect):
    outside = [name for name, (dk, dy) in _norm_ratios(ref.norm_case(257, 512), V5_ALPHA, defect).items() if not dk <= ref.MARGIN * dy]
    assert outside and set(outside) <= {"da", "dx"}, outside


def _gated_ratios(case, defect=None):
    exact, yard = ref.gated_torch(case), ref.gated_torch(case, dtype=torch.float16)
    got = ref.gated_formulas(case, emulate=True, defect=defect)
    return {n: (ref.dist(g, e), ref.dist(y, e)) for n, g, e, y in zip(ref.GATED_NAMES, got, exact, yard)}


@pytest.mark.parametrize("M,D,F", GATED_SHAPES)
def test_gated_emulation_is_inside_the_margin(M, D, F):
    for name, (dk, dy) in _gated_ratios(ref.gated_case(M, D, F)).items():
        print("gated M=%d D=%d F=%d %-2s: dist(emulation) = %.3e  dist(yardstick) = %.3e" % (M, D, F, name, dk, dy))
        assert dk <= ref.MARGIN * dy, name


@pytest.mark.parametrize("defect,hit", zip(ref.GATED_DEFECTS, ({"dx", "dw"}, {"h", "dx", "dw"}, {"dw"})))
def test_gated_defects_are_outside_the_margin(defect, hit):
    outside = {name for name, (dk, dy) in _gated_ratios(ref.gated_case(130, 128, 256), defect).items() if not dk <= ref.MARGIN * dy}
    assert outside == hit


def test_the_layer_restatement_is_the_oracles_forward():
    """layer_forward (the restatement the device tests differentiate) computes what oracle/nn_ref.py's transformer_layer_forward does."""
    from oracle import nn_ref
    from bonito_amd.transformer.model import TransformerEncoderLayer
    N, T, D, F, H, window = 2, 40, 128, 256, 2, (3, 5)
    case = ref.layer_case(N, T, D, F)
    layer = TransformerEncoderLayer(D, H, F, V5_ALPHA, 0.3, attn_window=window)
    layer.load_state_dict({k: case[k] for k in ref.LAYER_PARAMS}, strict=False)
    want = nn_ref.transformer_layer_forward(layer, case["x"].float())
    got = ref.layer_forward({k: v.double() for k, v in case.items()}, case["x"].double(), H, window, V5_ALPHA, ref.EPS, torch.float64)
    assert ref.dist(got, want) < 1e-5


# ---- refusals, on the CPU ------------------------------------------------------------------------------------------------------------------------
def test_norm_functions_refuse_before_any_launch():
    from bonito_amd import train_ops
    from bonito_amd.nn import NoTorchCompute
    c = ref.norm_case(4, 64)
    a, x, w, dy = c["a"], c["x"], c["w"], c["dy"]
    for fn, args in ((train_ops.rmsnorm_residual_forward, (a, x, w, 1.0)), (train_ops.rmsnorm_residual_backward, (a, x, w, dy, 1.0)),
                     (train_ops.rmsnorm_residual, (a.float(), x.float(), w, torch.tensor(1.0)))):
        with pytest.raises(NoTorchCompute, match="runs on a HIP device only"):
            fn(*args)
    for kw, text in ((dict(a=a.float()), "a must be float16"), (dict(x=x[:3]), "one shape"), (dict(w=w.half()), "must be float32"),
                     (dict(w=w[:32]), "weight must be"), (dict(alpha=float("nan")), "alpha must be finite"), (dict(eps=-1.0), "eps finite"),
                     (dict(a=a[:, :60], x=x[:, :60], w=w[:60]), "multiple of 8"), (dict(a=a[0], x=x[0]), "one shape"), (dict(a=None), "a must be a tensor"),
                     (dict(alpha=torch.ones(2)), "one number")):
        k = dict(a=a, x=x, w=w, alpha=1.0, eps=1e-5)
        k.update(kw)
        with pytest.raises(ValueError, match=text):
            train_ops.rmsnorm_residual_forward(k["a"], k["x"], k["w"], k["alpha"], k["eps"])
    big = torch.zeros(2, 1032, dtype=torch.float16)
    with pytest.raises(ValueError, match="8..1024"):
        train_ops.rmsnorm_residual(big, big, torch.ones(1032), 1.0)
    with pytest.raises(ValueError, match="dy must be float16"):
        train_ops.rmsnorm_residual_backward(a, x, w, dy.float(), 1.0)
    with pytest.raises(ValueError, match="dy must be float16"):
        train_ops.rmsnorm_residual_backward(a, x, w, dy[:3], 1.0)
    with pytest.raises(ValueError, match="a must be float16 or float32"):
        train_ops.rmsnorm_residual(a.double(), x, w, 1.0)


def test_gated_functions_refuse_before_any_launch():
    from bonito_amd import train_ops
    from bonito_amd.nn import NoTorchCompute
    c = ref.gated_case(6, 64, 72)
    x, w, dh = c["x"], c["w"], c["dh"]
    for fn, args in ((train_ops.gated_linear_forward, (x, w)), (train_ops.gated_linear_backward, (x, w, dh)), (train_ops.gated_linear, (x.float(), w))):
        with pytest.raises(NoTorchCompute, match="runs on a HIP device only"):
            fn(*args)
    for kw, text in ((dict(x=x.float()), "x must be float16"), (dict(w=w.half()), "must be float32"), (dict(w=w[:143]), r"weight must be \[2F\]\[D\]"),
                     (dict(w=w[:, :60]), "x must be"), (dict(w=w[:136]), "multiples of 8"), (dict(x=x[:, :60], w=w[:, :60]), "multiples of 8"),
                     (dict(w=w[0]), r"weight must be \[2F\]\[D\]"), (dict(x=x[0, 0]), "x must be"), (dict(x=None), "x must be a tensor")):
        k = dict(x=x, w=w)
        k.update(kw)
        with pytest.raises(ValueError, match=text):
            train_ops.gated_linear_forward(k["x"], k["w"])
    with pytest.raises(ValueError, match="dh must be float16"):
        train_ops.gated_linear_backward(x, w, dh.float())
    with pytest.raises(ValueError, match="dh must be float16"):
        train_ops.gated_linear_backward(x, w, dh[:, :64])
    with pytest.raises(ValueError, match="x must be float16 or float32"):
        train_ops.gated_linear(x.double(), w)


def test_encoder_layer_refuses_what_the_kernels_do_not_serve():
    from bonito_amd import attn
    from bonito_amd.nn import NoTorchCompute
    from bonito_amd.transformer.model import MultiHeadAttention, TransformerEncoderLayer
    x = torch.zeros(2, 5, 128, dtype=torch.float16)
    make = lambda D=128, H=2, F=256, window=(3, 5): TransformerEncoderLayer(D, H, F, 1.4142136, 0.5, attn_window=window)      # noqa: E731
    with pytest.raises(ValueError, match="expected a bonito_amd.transformer.model.TransformerEncoderLayer container, got MultiHeadAttention"):
        attn.encoder_layer(MultiHeadAttention(128, 2, attn_window=(3, 5)), x)
    with pytest.raises(ValueError, match="only head_dim 64 is served, got 32"):
        attn.encoder_layer(make(H=4), x)
    with pytest.raises(ValueError, match="finite window"):
        attn.encoder_layer(make(window=None), x)
    with pytest.raises(ValueError, match="too wide"):
        attn.encoder_layer(make(window=(300, 300)), x)
    with pytest.raises(ValueError, match="dim_feedforward must be a multiple of 8"):
        attn.encoder_layer(make(F=260), x)
    with pytest.raises(ValueError, match=r"x must be \[N\]\[T\]\[128\]"):
        attn.encoder_layer(make(), x[:, :, :64])
    layer = make()
    layer.self_attn.rotary_dim = 32
    with pytest.raises(ValueError, match="rotary_dim must equal head_dim"):
        attn.encoder_layer(layer, x)
    with pytest.raises(NoTorchCompute):
        attn.encoder_layer(make(), x)
    assert {"encoder_layer", "mha_module"} <= set(attn.__all__)


def test_forward_train_refusals_of_the_transformer_family():
    from bonito_amd.nn import NoTorchCompute
    from bonito_amd.transformer import Model
    x = ref.model_batch(2)[0]
    wide = ref.model_config()
    wide["model"]["encoder"]["transformer_encoder"]["layer"]["attn_window"] = [300, 300]
    odd = ref.model_config()
    odd["model"]["encoder"]["transformer_encoder"]["layer"]["dim_feedforward"] = 260
    narrow = ref.model_config()
    narrow["model"]["encoder"]["conv"]["sublayers"][2]["size"] = 64
    back = ref.model_config()
    back["model"]["encoder"]["upsample"]["batch_first"] = False
    for config, text in ((ref.model_config(norm="batchnorm"), r"layer 0 \(Convolution\) carries a norm \(batchnorm\)"),
                         (ref.model_config(time_major=True), r"layer 4 \(TransformerEncoderLayer\) follows the permute to time-major"),
                         (wide, r"layer 4 \(TransformerEncoderLayer\): window \(300, 300\) is too wide"),
                         (odd, r"layer 4 \(TransformerEncoderLayer\): dim_feedforward must be a multiple of 8"),
                         (narrow, r"layer 4 \(TransformerEncoderLayer\) has d_model 128 and follows 64 channels"),
                         (back, r"layer 6 \(LinearUpsample\) with batch_first=False has no training forward")):
        model = Model(config)
        with pytest.raises(ValueError, match=text):
            model.forward_train(x)
        assert model._hip is None
    model = Model(ref.model_config())
    with pytest.raises(ValueError, match=r"layer 0 \(Convolution\) holds float16 parameters"):
        Model(ref.model_config()).half().forward_train(x)
    with pytest.raises(NoTorchCompute, match="forward_train runs on a HIP device only"):      # everything else about it is served
        model.forward_train(x)
    assert model._hip is None


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree_on_the_new_entry_points():
    import ctypes as C
    from bonito_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bonito_hip.h")).read(), flags=re.S)
    ctype = {"const void*": C.c_void_p, "void*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p, "long": C.c_long, "int": C.c_int,
             "float": C.c_float, "size_t": C.c_size_t}
    names = sorted(n for n in _lib.SIGNATURES if n.startswith(("bh_rmsnorm_train_", "bh_gated_linear_train_")))
    assert names == ["bh_gated_linear_train_backward", "bh_gated_linear_train_forward", "bh_gated_linear_train_workspace",
                     "bh_rmsnorm_train_backward", "bh_rmsnorm_train_workspace"]
    handle = _lib.lib()
    for name in names:
        found = re.search(r"\b(size_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert found, "%s is not declared in include/bonito_hip.h" % name
        args = [ctype[re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*")] for a in found.group(2).split(",")]
        res, bound = _lib.SIGNATURES[name]
        assert res is ctype[found.group(1)] and bound == args, name
        assert hasattr(handle, name), "libbonito_hip.so does not export %s" % name
    # the workspace rules need no device: 0 for what is not served
    ws = handle.bh_rmsnorm_train_workspace
    assert ws(1, 8) > 0 and ws(257, 1024) >= 5 * 1024 * 4 and ws(257, 1024) == ws(257, 1024)
    assert ws(0, 64) == 0 and ws(4, 60) == 0 and ws(4, 1032) == 0 and ws(4, 0) == 0
    gw = handle.bh_gated_linear_train_workspace
    assert gw(17, 64, 72) >= 17 * 144 * 2 + 144 * 64 * (2 + 4)
    assert gw(0, 64, 72) == 0 and gw(4, 60, 72) == 0 and gw(4, 64, 68) == 0 and gw(2 ** 31, 8, 8) == 0

"""The references of batch-statistics BatchNorm (tests/batchnorm_train_ref.py) pinned on the CPU, and everything about the new layer that
needs no device: the refusals of bonito_amd.train_ops.batchnorm and SeqdistModel.forward_train(norm=...), and the C ABI.

    formulas == fp64 torch.nn.functional.batch_norm(training=True) + activation under autograd == central differences
    emulate (fp32 design, fp16 storage) within 2 dist(yardstick) per output and within the derived bound per statistic
    every planted defect outside its bound"""
import os
import re

import pytest
import torch

import batchnorm_train_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
ACTS = (None, "swish", "relu", "tanh")


def _mask(case, act, clamp):
    """The mask the emulation reads from its own fp16 y."""
    return ref.emulate(case, act, clamp)[0]


def _want(case, act, m):
    """exact, with the two statistics torch does not hand out taken from the formulas."""
    f = ref.formulas(case, act, m)
    return {**{k: f[k] for k in ("mean", "rstd")}, **ref.exact(case, act, m)}


# ---- the formulas -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("clamp", (None, ref.CLAMP))
def test_the_formulas_are_torchs_batch_norm_in_training_mode(act, clamp):
    case = ref.bn_case(3, 50, 16, offset_channel=5, constant_channel=9)
    m = _mask(case, act, clamp)
    f, t = ref.formulas(case, act, m), ref.exact(case, act, m)
    for name in ref.NAMES + ("running_mean", "running_var"):
        assert ref.dist(f[name], t[name]) < 1e-11, name
    # torch's unbiased running_var and momentum, stated once more by hand
    z = case["z"].to(F64).reshape(-1, 16)
    assert torch.allclose(t["running_var"], 0.9 * case["running_var"].to(F64) + 0.1 * z.var(0, unbiased=True), rtol=1e-12, atol=0)
    assert torch.allclose(t["running_mean"], 0.9 * case["running_mean"].to(F64) + 0.1 * z.mean(0), rtol=1e-12, atol=1e-15)


def test_the_formulas_without_affine_parameters_and_without_running_buffers():
    case = ref.bn_case(2, 9, 8)
    case.update(gamma=None, beta=None, running_mean=None, running_var=None)
    m = _mask(case, "swish", None)
    f, t = ref.formulas(case, "swish", m), ref.exact(case, "swish", m)
    assert ref.dist(f["y"], t["y"]) < 1e-11 and ref.dist(f["dz"], t["dz"]) < 1e-11
    assert t["dgamma"] is None and "running_mean" not in f and "running_mean" not in t


@pytest.mark.parametrize("act", ("swish", "tanh", None))
def test_the_formulas_against_central_differences(act):
    case = ref.bn_case(2, 7, 8, seed=3)
    m = torch.ones(2, 7, 8, dtype=torch.bool)
    f = ref.formulas(case, act, m)
    dy = case["dy"].to(F64)

    def loss(z=None, gamma=None, beta=None):
        c = dict(case)
        c.update({k: v for k, v in (("z", z), ("gamma", gamma), ("beta", beta)) if v is not None})
        zz, C = c["z"].to(F64), 8
        mean = zz.reshape(-1, C).mean(0)
        var = zz.reshape(-1, C).var(0, unbiased=False)
        u = c["gamma"].to(F64) * (zz - mean) / torch.sqrt(var + ref.EPS) + c["beta"].to(F64)
        return float((ref.act_fn(u, act) * dy).sum())

    h = 1e-6
    z64, g64, b64 = case["z"].to(F64), case["gamma"].to(F64), case["beta"].to(F64)
    for idx in ((0, 0, 0), (1, 3, 5), (1, 6, 7)):
        e = torch.zeros_like(z64)
        e[idx] = h
        assert abs((loss(z=z64 + e) - loss(z=z64 - e)) / (2 * h) - float(f["dz"][idx])) < 1e-6 * max(1.0, float(f["dz"].abs().max()))
    for c in (0, 5):
        e = torch.zeros(8, dtype=F64)
        e[c] = h
        assert abs((loss(gamma=g64 + e) - loss(gamma=g64 - e)) / (2 * h) - float(f["dgamma"][c])) < 1e-6 * float(f["dgamma"].abs().max())
        assert abs((loss(beta=b64 + e) - loss(beta=b64 - e)) / (2 * h) - float(f["dbeta"][c])) < 1e-6 * float(f["dbeta"].abs().max())


# ---- yardstick, emulation, defects ------------------------------------------------------------------------------------------------------------
def test_the_yardstick_is_about_a_thousandth_on_a_small_case():
    case = ref.bn_case(3, 50, 16)
    m = _mask(case, "swish", None)
    want, yard = ref.exact(case, "swish", m), ref.yardstick(case, "swish", m)
    for name in ref.NAMES:
        d = ref.dist(yard[name], want[name])
        print("yardstick 3x50x16 %-7s: dist = %.3e" % (name, d))
        assert 1e-4 < d < 1e-2, (name, d)


EMULATED = ((3, 50, 16, "swish", None, {}), (3, 50, 16, "swish", ref.CLAMP, dict(offset_channel=5, constant_channel=9)),
            (1, 2, 8, "tanh", None, {}), (2, 257, 64, "relu", ref.CLAMP, dict(offset_channel=63)), (5, 1000, 8, None, None, dict(constant_channel=0)))


@pytest.mark.parametrize("N,L,C,act,clamp,kw", EMULATED)
def test_the_emulated_design_is_inside_every_bound(N, L, C, act, clamp, kw):
    case = ref.bn_case(N, L, C, **kw)
    m, got = ref.emulate(case, act, clamp)
    want, yard = _want(case, act, m), ref.yardstick(case, act, m)
    bounds = ref.stat_bounds(case["z"], case["running_mean"], case["running_var"])
    for name in ref.NAMES:
        dk, dy = ref.dist(got[name] * m if name == "y" else got[name], want[name]), ref.dist(yard[name], want[name])
        print("emulate %dx%dx%d %-7s: dist = %.3e  yardstick = %.3e  ratio = %.3f" % (N, L, C, name, dk, dy, dk / dy if dy else 0.0))
    for name in ref.STATS:
        err = (got[name].to(F64) - want[name]).abs()
        print("emulate %dx%dx%d %-12s: max error / bound = %.3f" % (N, L, C, name, float((err / bounds[name]).max())))
    assert ref.outside(got, want, yard, bounds, m) == []
    assert bool(torch.isfinite(got["dz"].float()).all())


def test_the_bound_of_the_statistics_is_a_formula_in_m_and_the_partial_size():
    assert ref.block_rows(2) == 64 and ref.block_rows(64 * 2048) == 64 and ref.block_rows(64 * 2048 + 1) == 65
    assert ref.depth(2) == 64 + 256 + 1 + 8 and ref.depth(768000) == 375 + 256 + 256 + 8
    case = ref.bn_case(3, 50, 16)
    b = ref.stat_bounds(case["z"], case["running_mean"], case["running_var"])
    assert all(bool((b[name] > 0).all()) for name in ref.STATS)
    assert float(b["mean"].max()) < 1e-4 and float(b["running_var"].max()) < 1e-4        # far below what a defect moves


@pytest.mark.parametrize("defect", ref.DEFECTS)
def test_every_planted_defect_is_outside_its_bound(defect):
    # channel 5 has mean 8 and standard deviation 0.05: the case raw moments in fp32 and a missing eps cannot pass
    case = ref.bn_case(3, 50, 16, offset_channel=5)
    m, got = ref.emulate(case, "swish", None, defect=defect)
    want, yard = _want(case, "swish", m), ref.yardstick(case, "swish", m)
    bad = ref.outside(got, want, yard, ref.stat_bounds(case["z"], case["running_mean"], case["running_var"]), m)
    print("%-22s outside: %s" % (defect, ", ".join(bad)))
    expected = {"biased_running_var": "running_var", "xhat_term_dropped": "dz", "dbeta_term_dropped": "dz", "M_taken_as_L": "mean",
                "eps_missing": "rstd", "act_grad_at_z": "dz", "gamma_missing_from_dz": "dz", "raw_moments": "rstd"}[defect]
    assert expected in bad, (defect, bad)


# ---- refusals, before any launch ----------------------------------------------------------------------------------------------------------------
def test_batchnorm_functions_refuse_before_any_launch():
    from bonito_amd import train_ops
    from bonito_amd.nn import NoTorchCompute
    c = ref.bn_case(3, 5, 16)
    z, g, b, rm, rv, dy = c["z"], c["gamma"], c["beta"], c["running_mean"], c["running_var"], c["dy"]
    mean, rstd = torch.zeros(16), torch.ones(16)
    for fn, args in ((train_ops.batchnorm_forward, (z, g, b, rm, rv)), (train_ops.batchnorm_backward, (z, g, b, mean, rstd, z, dy)),
                     (train_ops.batchnorm, (z.float(), g, b, rm, rv)), (train_ops.batchnorm, (z, None, None))):
        with pytest.raises(NoTorchCompute, match="runs on a HIP device only"):
            fn(*args)
    for kw, text in ((dict(z=z.float()), "z must be float16"), (dict(z=z[0]), r"z must be \[N\]\[L\]\[C\]"), (dict(z=None), "z must be a tensor"),
                     (dict(z=z[:, :, :12], weight=g[:12], bias=b[:12]), "multiple of 8"), (dict(weight=g.half()), "must be float32"),
                     (dict(weight=g[:8]), r"weight must be \(16,\)"), (dict(bias=None), "weight and bias come together"),
                     (dict(z=z[:1, :1]), "more than one value per channel"), (dict(channels=17), r"channels must be in 1\.\.16"),
                     (dict(channels=0), r"channels must be in 1\.\.16"), (dict(running_var=None), "running_mean and running_var come together"),
                     (dict(running_mean=rm[:12], running_var=rv[:12]), r"running_mean must be \(16,\)"),
                     (dict(channels=12), r"running_mean must be \(12,\)"), (dict(running_mean=rm.double()), "must be float32"),
                     (dict(momentum=None), "momentum=None"), (dict(momentum=1.5), r"momentum must be in 0\.\.1"),
                     (dict(eps=0.0), "eps must be finite and > 0"), (dict(eps=float("nan")), "eps must be finite and > 0"),
                     (dict(activation="gelu"), "activation 'gelu' is not supported"), (dict(clamp=(1.0, -1.0)), "clamp range")):
        k = dict(z=z, weight=g, bias=b, running_mean=rm, running_var=rv, momentum=0.1, eps=1e-5, activation="swish", clamp=None, channels=None)
        k.update(kw)
        with pytest.raises(ValueError, match=text):
            train_ops.batchnorm_forward(**k)
    with pytest.raises(ValueError, match="dy must be float16"):
        train_ops.batchnorm_backward(z, g, b, mean, rstd, z, dy.float())
    with pytest.raises(ValueError, match="y must be float16"):
        train_ops.batchnorm_backward(z, g, b, mean, rstd, z.permute(1, 0, 2), dy)          # batch-major y where time_major is off
    with pytest.raises(ValueError, match=r"mean must be \(16,\)"):
        train_ops.batchnorm_backward(z, g, b, mean[:8], rstd, z, dy)
    with pytest.raises(ValueError, match="z must be float16 or float32"):
        train_ops.batchnorm(z.double(), g, b)
    assert {"batchnorm_forward", "batchnorm_backward", "batchnorm"} <= set(train_ops.__all__)


def _model(config=None):
    from bonito_amd.crf.model import Model
    return Model(config or ref.lstm_config())


def test_forward_train_refusals_of_normalised_convolutions():
    from bonito_amd import nn as bnn
    from bonito_amd.nn import NoTorchCompute
    x = torch.zeros(2, 1, 100, dtype=torch.float16)
    model = _model().train()
    with pytest.raises(ValueError, match=r"layer 0 \(Convolution\) carries a norm \(batchnorm\); a normalised convolution has no training "
                                         "backward yet"):
        model.forward_train(x)                                            # norm=None: today's message, word for word
    with pytest.raises(ValueError, match=r"layer 0 \(Convolution\) carries a norm \(batchnorm\) and norm='frozen' is not served"):
        model.forward_train(x, norm="frozen")
    with pytest.raises(ValueError, match=r"layer 0 \(Convolution\) has its BatchNorm in eval mode"):
        _model().eval().forward_train(x, norm="batch")
    half_eval = _model().train()
    list(half_eval.encoder.children())[1].norm.bn.eval()
    with pytest.raises(ValueError, match=r"layer 1 \(Convolution\) has its BatchNorm in eval mode"):
        half_eval.forward_train(x, norm="batch")
    cumulative = _model().train()
    list(cumulative.encoder.children())[2].norm.bn.momentum = None
    with pytest.raises(ValueError, match=r"layer 2 \(Convolution\) has a BatchNorm with momentum=None"):
        cumulative.forward_train(x, norm="batch")
    other = _model().train()
    list(other.encoder.children())[0].norm = bnn.Clamp(-1.0, 1.0)
    with pytest.raises(ValueError, match=r"layer 0 \(Convolution\) carries a norm \(clamp\) that is no BatchNorm"):
        other.forward_train(x, norm="batch")
    with pytest.raises(ValueError, match=r"layer 2 \(Convolution\) normalises 1 value per channel"):
        model.forward_train(torch.zeros(1, 1, 5, dtype=torch.float16), norm="batch")
    odd = ref.lstm_config()
    odd["encoder"]["sublayers"][2]["size"] = 36                           # 36 channels in front of the permute: nothing pads them
    with pytest.raises(ValueError, match=r"layer 2 \(Convolution\) normalises 36 channels"):
        _model(odd).train().forward_train(x, norm="batch")
    plain = ref.lstm_config()
    for layer in plain["encoder"]["sublayers"][:3]:
        del layer["norm"]
    with pytest.raises(ValueError, match="norm='bogus' is not served"):
        _model(plain).forward_train(x, norm="bogus")
    with pytest.raises(ValueError, match=r"layer 0 \(Convolution\) holds float16 parameters"):
        _model().half().train().forward_train(x, norm="batch")
    before = {k: v.clone() for k, v in model.state_dict().items()}
    with pytest.raises(NoTorchCompute, match="forward_train runs on a HIP device only"):       # everything else about it is served
        model.forward_train(x, norm="batch")
    assert model._hip is None and all(torch.equal(v, before[k]) for k, v in model.state_dict().items())


def test_trainer_and_command_line_take_the_keyword():
    import inspect
    from bonito_amd.cli import train as cli
    from bonito_amd.training import Trainer
    assert inspect.signature(Trainer.__init__).parameters["norm"].default is None
    args = cli.argparser().parse_args(["out", "--norm", "batch"])
    assert args.norm == "batch" and cli.argparser().parse_args(["out"]).norm is None
    with pytest.raises(SystemExit):
        cli.argparser().parse_args(["out", "--norm", "frozen"])


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree_on_the_new_entry_points():
    import ctypes as C
    from bonito_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bonito_hip.h")).read(), flags=re.S)
    ctype = {"const void*": C.c_void_p, "void*": C.c_void_p, "const float*": C.c_void_p, "float*": C.c_void_p, "long": C.c_long, "int": C.c_int,
             "float": C.c_float, "size_t": C.c_size_t}
    names = sorted(n for n in _lib.SIGNATURES if n.startswith("bh_batchnorm_train_"))
    assert names == ["bh_batchnorm_train_backward", "bh_batchnorm_train_forward", "bh_batchnorm_train_workspace"]
    handle = _lib.lib()
    for name in names:
        found = re.search(r"\b(size_t|int)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert found, "%s is not declared in include/bonito_hip.h" % name
        args = [ctype[re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*")] for a in found.group(2).split(",")]
        res, bound = _lib.SIGNATURES[name]
        assert res is ctype[found.group(1)] and bound == args, name
        assert hasattr(handle, name), "libbonito_hip.so does not export %s" % name
    kernels = open(os.path.join(ROOT, "bonito_amd", "csrc", "kernels.h")).read()
    assert all("bh_k_" + name[3:] in kernels for name in names)
    # the workspace rules need no device: 0 for what is not served, two partial sums per block and channel otherwise
    ws = handle.bh_batchnorm_train_workspace
    assert ws(1, 2, 8) >= 2 * 8 * 4 and ws(5, 1000, 520) >= 2 * -(-5000 // ref.block_rows(5000)) * 520 * 4 and ws(3, 5, 16) == ws(3, 5, 16)
    assert ws(1, 1, 8) == 0 and ws(0, 5, 8) == 0 and ws(3, 5, 12) == 0 and ws(3, 5, 2056) == 0 and ws(3, 0, 8) == 0
    assert ws(64, 12000, 64) >= 2 * -(-768000 // ref.block_rows(768000)) * 64 * 4

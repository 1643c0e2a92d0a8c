"""SeqdistModel.forward_train(x, norm="batch"), Trainer(norm="batch") and ``train --norm batch`` on the device (-m gpu): models whose
convolutions carry a BatchNorm, as every published configuration does - a 32-feature LSTM-family model and a small v5-style
transformer model (tests/batchnorm_train_ref.py: lstm_config, and transformer_train_ref.model_config(norm="batchnorm")), their running
statistics randomised by synthetic.randomise_batchnorm_.

Against a torch restatement of the encoder with torch's own batch norm in training mode (lstm_model_torch, v5_model_torch): exact = fp64,
yardstick = the same in fp16 on the CPU, the upstream gradient d loss / d scores captured by a hook. Every parameter gradient, gamma and
beta included, and every running statistic must satisfy dist(kernel) <= 2 dist(yardstick), the rule of the existing model tests; scores
are within the 1e-2 those tests allow a forward. A convolution's bias in front of a batch norm has a gradient that is identically zero,
which no relative distance can be taken from: the device's value is held below the rounding of its fp16 dz, 2^-11 sum |dz| per channel.
The LSTM-family model is the existing model test's, weights included (train_layers_ref.chain_params), with the norms added. Inference after training (the engine dropped, eval mode) is the restatement in eval mode
on the NEW statistics - and is not the one on the old ones."""
import functools
import os
import re

import pytest
import torch

import batchnorm_train_ref as ref
import conftest
import test_gpu_train_cli as cli
import test_gpu_train_model as tm
import train_layers_ref as tl
import transformer_train_ref as tt
from bonito_amd import optim, synthetic, util
from bonito_amd.__main__ import main
from bonito_amd.crf.model import Model
from bonito_amd.training import Trainer
from bonito_amd.transformer import Model as TransformerModel

pytestmark = pytest.mark.gpu

DEV = "cuda"
FORWARD = 1e-2          # dist(scores, fp64 restatement) the existing model tests allow a forward in fp16


def _make(kind, seed):
    """Seeded; the LSTM-family model carries the weights the existing model test trains (train_layers_ref.chain_params). gamma and beta
    are moved off 1 and 0, the running statistics off 0 and 1."""
    torch.manual_seed(seed)
    model = Model(ref.lstm_config()) if kind == "lstm" else TransformerModel(tt.model_config(norm="batchnorm"))
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        if kind == "lstm":
            named = dict(model.encoder.named_parameters())
            for name, (_, value) in zip(ref.lstm_model_names(), tl.chain_params(32, 4, 5, 19, 5, 256)):       # that test's weights, as they are
                named[name].copy_(value)
        for name, p in model.encoder.named_parameters():
            if "norm.bn." in name:
                p.copy_((1.0 if name.endswith("weight") else 0.0) + 0.3 * torch.randn(p.shape, generator=g))
    synthetic.randomise_batchnorm_(model, seed + 1)
    return model.to(DEV).train()


def _state(model):
    params = {k: v.detach().cpu().clone() for k, v in model.encoder.named_parameters()}
    buffers = {k: v.detach().cpu().clone() for k, v in model.encoder.named_buffers()}
    return params, buffers


def _restate(kind, params, buffers, signal, mask, dscores=None, dtype=torch.float64, training=True):
    if kind == "lstm":
        return ref.lstm_model_torch(params, buffers, signal, dscores, dtype, training)
    return ref.v5_model_torch(params, buffers, signal, mask, dscores, dtype, training)


def _mask(kind, scores):
    lo, hi = tt.MODEL["clamp"]
    s = scores.detach().float().cpu()
    return torch.ones_like(s, dtype=torch.bool) if kind == "lstm" else (s > lo) & (s < hi)


@functools.lru_cache(maxsize=None)
def _run(kind):
    """One forward_train(norm="batch") -> loss -> backward, with the captured upstream gradient and the state before it."""
    model = _make(kind, 4)
    x, targets, lengths = tm._batch(3) if kind == "lstm" else tt.model_batch(3)
    params, buffers = _state(model)
    captured = []
    scores = model.forward_train(x.to(DEV), norm="batch")
    scores.register_hook(captured.append)
    loss = model.loss(scores, targets, lengths)
    loss.backward()
    torch.cuda.synchronize()
    return model, params, buffers, x, scores.detach(), captured[0].detach().cpu()


@pytest.mark.parametrize("kind", ("lstm", "v5"))
def test_scores_gradients_and_statistics_against_the_restatement(kind):
    model, params, buffers, x, scores, dscores = _run(kind)
    mask = _mask(kind, scores)
    y64, exact, buf64 = _restate(kind, params, buffers, x[:, 0], mask, dscores)
    _, yard, buf16 = _restate(kind, params, buffers, x[:, 0], mask, dscores, dtype=torch.float16)
    d = ref.dist(scores, y64)
    print("%s forward_train(norm=batch) against fp64: dist = %.3e" % (kind, d))
    assert scores.dtype == torch.float16 and scores.shape == y64.shape and d < FORWARD
    failed = []
    named = dict(model.encoder.named_parameters())
    assert {k for k in exact if not k.endswith("conv.z")} == {k for k, p in named.items() if p.requires_grad}
    assert any("norm.bn.weight" in k for k in exact)
    for name in exact:
        if name.endswith("conv.z"):
            continue
        g = named[name].grad
        assert g is not None and g.dtype == torch.float32 and g.shape == named[name].shape, name
        if name.endswith("conv.bias"):
            # in front of a batch norm the exact gradient is sum_m dz = 0 identically (fp64 leaves 1e-15 of it): there is no relative
            # distance from it. The device's value is the rounding of its fp16 dz, summed in fp32: |db_c| <= 2^-11 sum_m |dz_mc|, with
            # 1 % for the distance of the device's dz from the exact one
            bound = 2.0 ** -11 * 1.01 * exact[name[:-4] + "z"].abs().sum((0, 2))
            worst = float((g.cpu().double().abs() / bound).max())
            print("%s %-40s: max |gradient| = %.3e against exactly 0; largest |db| / (2^-11 sum |dz|) = %.3f" % (kind, name, float(g.abs().max()), worst))
            assert float(exact[name].abs().max()) < 1e-9 * float(bound.max()), name
            if not worst <= 1.0:
                failed.append((name, worst, 1.0))
            continue
        dk, dy = ref.dist(g, exact[name]), ref.dist(yard[name], exact[name])
        print("%s %-40s: dist(kernel) = %.3e  dist(yardstick) = %.3e  ratio = %.3f" % (kind, name, dk, dy, dk / dy))
        if not dk <= ref.MARGIN * dy:
            failed.append((name, dk, dy))
    for name, b in model.encoder.named_buffers():
        if "norm.bn." not in name:
            continue
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(buffers[name]) + 1, name
            continue
        assert not torch.equal(b.cpu(), buffers[name]), name                       # the forward rewrote it
        dk, dy = ref.dist(b, buf64[name]), ref.dist(buf16[name], buf64[name])
        print("%s %-40s: dist(kernel) = %.3e  dist(yardstick) = %.3e  ratio = %.3f" % (kind, name, dk, dy, dk / dy))
        if not dk <= ref.MARGIN * dy:
            failed.append((name, dk, dy))
    assert not failed, failed
    assert model._hip is None                                                       # forward_train builds no engine


@pytest.mark.parametrize("kind", ("lstm", "v5"))
def test_three_steps_of_statistics_and_the_inference_that_follows(kind):
    model = _make(kind, 6)
    batches = [(tm._batch if kind == "lstm" else tt.model_batch)(4, seed=30 + i)[0] for i in range(4)]
    params, before = _state(model)
    stale = model.eval()(batches[3].to(DEV)).clone()                                # builds the engine on the old statistics
    model.train()
    ref64, ref16 = dict(before), dict(before)
    for x in batches[:3]:
        with torch.no_grad():                                                       # the statistics move under no_grad too, as in torch
            scores = model.forward_train(x.to(DEV), norm="batch")
        mask = _mask(kind, scores)
        ref64 = _restate(kind, params, ref64, x[:, 0], mask)[2]
        ref16 = _restate(kind, params, ref16, x[:, 0], mask, dtype=torch.float16)[2]
    failed = []
    for name, b in model.encoder.named_buffers():
        if "norm.bn." not in name:
            continue
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(before[name]) + 3, name
            continue
        dk, dy = ref.dist(b, ref64[name]), ref.dist(ref16[name], ref64[name])
        print("%s three steps %-36s: dist(kernel) = %.3e  dist(yardstick) = %.3e  ratio = %.3f" % (kind, name, dk, dy, dk / dy))
        if not dk <= ref.MARGIN * dy:
            failed.append((name, dk, dy))
    assert not failed, failed
    # inference: the engine of before holds the old statistics until it is dropped
    x = batches[3]
    model.eval()
    assert torch.equal(model(x.to(DEV)), stale)
    model._drop_engine()
    fresh = model(x.to(DEV))
    mask = _mask(kind, fresh)
    after = {k: v.detach().cpu() for k, v in model.encoder.named_buffers()}
    new64 = _restate(kind, params, after, x[:, 0], mask, training=False)[0]
    old64 = _restate(kind, params, before, x[:, 0], mask, training=False)[0]
    d_new, d_old = ref.dist(fresh, new64), ref.dist(fresh, old64)
    print("%s eval after training: dist to the restatement on the new statistics = %.3e, on the old ones = %.3e" % (kind, d_new, d_old))
    assert d_new < FORWARD < d_old
    with pytest.raises(ValueError, match="has its BatchNorm in eval mode"):
        model.forward_train(x.to(DEV), norm="batch")


def test_what_only_the_layout_tells_is_refused_before_the_statistics_are_touched():
    """The five encoders of batchnorm_train_ref.misbuilt_models on the device: each begins with a normalised convolution, which a refusal
    behind the first launch would already have run. The refusal names the layer and the three BatchNorm buffers keep their bits."""
    x = torch.zeros(2, 1, 120, dtype=torch.float16, device=DEV)
    for name, model, text in ref.misbuilt_models():
        synthetic.randomise_batchnorm_(model, 3)
        model = model.to(DEV).train()
        before = ref.batchnorm_buffers(model)
        assert len(before) == 3, name
        with pytest.raises(ValueError, match=text):
            model.forward_train(x, norm="batch")
        torch.cuda.synchronize()
        after = ref.batchnorm_buffers(model)
        assert all(torch.equal(before[k].reshape(-1).view(torch.uint8), after[k].reshape(-1).view(torch.uint8)) for k in before), name


@pytest.mark.parametrize("kind", ("lstm", "v5"))
def test_twenty_adamw_steps_lower_the_loss(kind):
    model = _make(kind, 2)
    x, targets, lengths = (tm._batch if kind == "lstm" else tt.model_batch)(8, seed=9)
    x = x.to(DEV)
    opt = optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=2e-3)
    losses = []
    for step in range(21):
        opt.zero_grad(set_to_none=True)
        loss = model.loss(model.forward_train(x, norm="batch"), targets, lengths)
        losses.append(float(loss.detach()))
        if step < 20:
            opt.scale(loss).backward()
            opt.step(2.0)
    print("%s losses: %s" % (kind, " ".join("%.4f" % v for v in losses)))
    assert all(v == v and abs(v) != float("inf") for v in losses) and losses[-1] < losses[0]
    tracked = [int(b) for n, b in model.named_buffers() if n.endswith("num_batches_tracked")]
    assert tracked == [21] * 3


def test_trainer_updates_the_statistics_once_per_sub_batch():
    model = _make("lstm", 8)
    x, targets, lengths = tm._batch(8, seed=9)
    batch = (x.float(), targets, lengths)
    with pytest.raises(ValueError, match=r"layer 0 \(Convolution\) carries a norm \(batchnorm\); a normalised convolution has no training"):
        plain = Trainer(model, DEV, [batch], [batch], chunks_per_epoch=8, batch_size=8)
        plain.init_optimizer(2e-3)
        plain.train_one_step(batch)
    trainer = Trainer(model, DEV, [batch], [batch], chunks_per_epoch=8, batch_size=8, grad_accum_split=2, norm="batch")
    trainer.init_optimizer(2e-3)
    before = {k: v.clone() for k, v in model.named_buffers()}
    losses, grad_norm, scale = trainer.train_one_step(batch)
    assert losses["loss"] == losses["loss"] and scale > 0
    for name, b in model.named_buffers():
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(before[name]) + 2, name
        else:
            assert not torch.equal(b, before[name]), name
    loss, mean_acc, median_acc = trainer.validate_one_epoch()                       # drops the engine: validation folds the new statistics
    assert loss == loss and not model.training


# ---- the command line ---------------------------------------------------------------------------------------------------------------------------
COMMON = cli.COMMON


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """data directory, a config with norm = "batchnorm" on every convolution and the uninterrupted two-epoch run (child process)."""
    root = tmp_path_factory.mktemp("train_norm_cli")
    data = root / "data"
    cli._write_chunks(str(data), 32, seed=21)
    cli._write_chunks(str(data / "validation"), 8, seed=22)
    cfg = root / "cfg.toml"
    with open(cfg, "w") as fh:
        util.dump_toml(ref.lstm_config(), fh)
    out = root / "run"
    done = cli._child("train", out, "--config", cfg, "--directory", data, "--norm", "batch", *COMMON)
    print(done.stdout, done.stderr)
    assert done.returncode == 0, done.stderr + done.stdout
    return dict(root=root, data=data, cfg=cfg, out=out, stdout=done.stdout)


def test_cli_run_trains_the_statistics_and_evaluates(run):
    out = run["out"]
    config = util.load_toml(out / "config.toml")
    assert config["training"]["norm"] == "batch" and config["encoder"]["sublayers"][0]["norm"] == "batchnorm"
    fresh = Model(ref.lstm_config()).state_dict()
    for epoch, steps in ((1, 4), (2, 8)):
        state = torch.load(out / ("weights_%d.tar" % epoch), map_location="cpu")
        for name in ("encoder.0.norm.bn.running_mean", "encoder.1.norm.bn.running_var", "encoder.2.norm.bn.running_mean"):
            assert bool(torch.isfinite(state[name]).all()) and not torch.equal(state[name], fresh[name]), name
        assert int(state["encoder.0.norm.bn.num_batches_tracked"]) == steps
    lines = re.findall(r"^\[epoch (\d)\] directory=\S+ loss=(\S+) mean_acc=(\S+)% median_acc=(\S+)%$", run["stdout"], flags=re.M)
    assert [int(m[0]) for m in lines] == [1, 2]
    done = cli._child("evaluate", out, "--directory", run["data"], "--chunks", "8", "--weights", "2", "--batchsize", "8")
    assert done.returncode == 0, done.stderr
    found = re.search(r"^\* loss mean\s+(\S+)$", done.stdout, flags=re.M)
    print("evaluate: loss mean %s; the epoch line: loss=%s" % (found.group(1), lines[1][1]))
    assert abs(float(found.group(1)) - float(lines[1][1])) <= 1e-3              # validation saw the trained statistics, as evaluate does


def test_a_resumed_run_ends_with_the_bytes_of_the_uninterrupted_one(run, capsys):
    out = run["root"] / "resumed"
    base = ["train", str(out), "--config", str(run["cfg"]), "--directory", str(run["data"]), "--norm", "batch"]
    one = [a if a != "2" else "1" for a in COMMON[:2]] + COMMON[2:]
    assert main(base + one) == 0
    assert main(base + COMMON + ["-f", "--restore-optim"]) == 0
    assert "[picking up weights, optim state from epoch 1]" in capsys.readouterr().out

    def flat(obj, prefix=""):
        if isinstance(obj, dict):
            return {k2: v2 for k, v in obj.items() for k2, v2 in flat(v, "%s/%s" % (prefix, k)).items()}
        if isinstance(obj, (list, tuple)):
            return {k2: v2 for i, v in enumerate(obj) for k2, v2 in flat(v, "%s/%d" % (prefix, i)).items()}
        return {prefix: obj}

    for name in ("weights_2.tar", "optim_2.tar"):
        a, b = (flat(torch.load(d / name, map_location="cpu")) for d in (run["out"], out))
        assert list(a) == list(b) and len(a) > 10
        assert name != "weights_2.tar" or sum(k.endswith(("running_mean", "running_var", "num_batches_tracked")) for k in a) == 9
        for key in a:
            if isinstance(a[key], torch.Tensor):
                assert a[key].dtype == b[key].dtype and a[key].numpy().tobytes() == b[key].numpy().tobytes(), (name, key)


def test_pretrained_runs_and_the_probe_leaves_every_buffer_alone(run, capsys, monkeypatch):
    from bonito_amd.cli import train as train_cli
    seen = {}

    class Stub:
        def __init__(self, model, *args, **kwargs):
            seen["state"] = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
            seen["training"], seen["norm"] = model.training, kwargs.get("norm")

        def fit(self, *args, **kwargs):
            pass

    base = ["--pretrained", str(run["out"]), "--directory", str(run["data"]), "--norm", "batch", "--epochs", "1"] + COMMON[2:]
    with monkeypatch.context() as patched:                                           # the run up to the Trainer: the probe has run
        patched.setattr(train_cli, "Trainer", Stub)
        assert main(["train", str(run["root"] / "probed")] + base) == 0
    saved = torch.load(run["out"] / "weights_2.tar", map_location="cpu")
    assert seen["norm"] == "batch" and not seen["training"] and set(seen["state"]) == set(saved)
    for key, value in saved.items():
        assert seen["state"][key].numpy().tobytes() == value.numpy().tobytes(), key
    capsys.readouterr()
    out = run["root"] / "finetuned"
    assert main(["train", str(out)] + base) == 0                                     # ... and the whole of it
    assert "[using pretrained model %s]" % run["out"] in capsys.readouterr().out
    state = torch.load(out / "weights_1.tar", map_location="cpu")
    assert int(state["encoder.0.norm.bn.num_batches_tracked"]) == 8 + 4
    assert not torch.equal(state["encoder.2.norm.bn.running_mean"], saved["encoder.2.norm.bn.running_mean"])
    refused = run["root"] / "refused"
    with pytest.raises(SystemExit) as exc:                                           # without the option: today's refusal, in front of any file
        main(["train", str(refused), "--pretrained", str(run["out"]), "--directory", str(run["data"])] + COMMON)
    assert exc.value.code == 1 and "carries a norm (batchnorm)" in capsys.readouterr().out and os.listdir(refused) == []
    assert conftest.ROOT

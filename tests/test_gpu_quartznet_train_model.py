"""bonito_amd.ctc.Model.forward_train, the Trainer and ``python -m bonito_amd train --norm batch`` on a QuartzNet CTC model, on the device
(-m gpu): the quartz_small fixture's configuration (conftest.load_ctc_fixture: three chunks of 600 samples), as it is (dropout 0.05 in
every block) and with every dropout set to 0.

The encoder is restated below in torch: torch's own depthwise convolution and batch norm, the dropout masks from the restatement's keep
function (tests/quartznet_train_ref.py) at the model's sites. exact = the restatement in fp64; yardstick = the restatement with fp16
operands and every result and gradient rounded to fp16 (ref.round16: what torch's fp16 kernels compute; torch's CPU grouped convolution
has no usable fp16 backward). With dist(a) = max|a - exact| / max|exact|, the log-probabilities, every parameter gradient (of a fixed
cotangent G on the log-probabilities, so that no loss is restated) and the running statistics must satisfy
dist(device) <= 2 dist(yardstick). Every figure is printed first."""
import csv
import os
import re

import pytest
import torch
import torch.nn.functional as F

import conftest
import quartznet_train_ref as ref
import test_gpu_train_cli as cli
import test_gpu_train_model as tm
from bonito_amd import optim, util
from bonito_amd.__main__ import main
from bonito_amd.ctc import Model
from bonito_amd.training import Trainer

pytestmark = pytest.mark.gpu

DEV = "cuda"
F64 = torch.float64
SEED = 0x0F1E2D3C4B5A6978
COMMON = cli.COMMON


def _config(dropout=None):
    cfg = conftest.load_ctc_fixture()[0]
    if dropout is None:
        return cfg
    return {**cfg, "block": [{**b, "dropout": dropout} for b in cfg["block"]]}


def _make(dropout=None):
    cfg, sd, x, _ = conftest.load_ctc_fixture()
    model = Model(_config(dropout))
    model.load_state_dict(sd)
    return model.to(DEV).train(), x.half()


def _restate(cfg, params, buffers, x, seed, dtype, rnd=lambda t: t, training=True):
    """-> (log-probabilities [T][N][classes], the buffers after the call). params: leaf tensors of `dtype` by state_dict name; x [N][1][L]."""
    act = {"swish": F.silu, "relu": torch.relu, "tanh": torch.tanh}[cfg["encoder"]["activation"]]
    buffers = {k: v.clone() for k, v in buffers.items()}
    site = [0]

    def drop(h, p):
        sid = site[0]
        site[0] += 1
        if not training or p == 0.0:
            return h
        N, C, L = h.shape
        mask = ref.keep_mask(seed, sid, N * L * C, p).reshape(N, L, C).permute(0, 2, 1)
        return rnd(h * mask.to(dtype) / (1.0 - p))

    def tcs_bn(prefix, bn, h, layer, separable, plain_stride=1):
        if separable:
            w = rnd(params[prefix + ".depthwise.weight"])
            h = rnd(F.conv1d(h, w, padding=w.shape[2] // 2, groups=w.shape[0]))
            h = rnd(F.conv1d(h, rnd(params[prefix + ".pointwise.weight"])))
        else:
            w = rnd(params[prefix + ".conv.weight"])
            h = rnd(F.conv1d(h, w, stride=plain_stride, padding=w.shape[2] // 2))
        rm, rv = buffers[bn + ".running_mean"].to(dtype), buffers[bn + ".running_var"].to(dtype)
        h = rnd(F.batch_norm(h, rm, rv, params[bn + ".weight"], params[bn + ".bias"], training=training, momentum=0.1, eps=1e-3))
        buffers[bn + ".running_mean"], buffers[bn + ".running_var"] = rm, rv
        return h

    h = x.to(dtype)
    for i, layer in enumerate(cfg["block"]):
        name, inp = "encoder.encoder.%d" % i, h
        for r in range(layer["repeat"]):
            h = tcs_bn("%s.conv.%d" % (name, 4 * r), "%s.conv.%d" % (name, 4 * r + 1), h, layer, layer["separable"], layer["stride"][0])
            if r < layer["repeat"] - 1:
                h = drop(rnd(act(h)), layer["dropout"])
        if layer["residual"]:
            h = rnd(h + tcs_bn(name + ".residual.0", name + ".residual.1", inp, layer, False))
        h = drop(rnd(act(h)), layer["dropout"])
    lp = rnd(torch.log_softmax(rnd(F.conv1d(h, rnd(params["decoder.layers.0.weight"]), rnd(params["decoder.layers.0.bias"]))), dim=1))
    return lp.permute(2, 0, 1), buffers


def _leaves(model, dtype):
    params = {k: v.detach().cpu().to(dtype).requires_grad_() for k, v in model.named_parameters()}
    buffers = {k: v.detach().cpu().clone() for k, v in model.named_buffers()}
    return params, buffers


def _cotangent(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(77)).half()


def test_a_first_convolution_wider_than_256_filters(dropout=0.0):
    """dna_r9.4.1@v2's first layer has 344 filters, the single-channel training convolution serves 256: forward_train pads the signal
    with seven zero channels. The fixture's configuration with 264 filters in its first block (seeded weights), every gradient as below."""
    cfg = _config(dropout)
    cfg = {**cfg, "block": [{**cfg["block"][0], "filters": 264}] + cfg["block"][1:]}
    torch.manual_seed(11)
    model, x = Model(cfg).to(DEV).train(), conftest.load_ctc_fixture()[2].half()
    _gradients(model, cfg, x, "quartz_small, 264 first filters")


@pytest.mark.parametrize("dropout", [None, 0.0])
def test_forward_train_and_every_gradient_against_the_restatement(dropout):
    model, x = _make(dropout)
    cfg = _config(dropout)
    lp = _gradients(model, cfg, x, "quartz_small dropout=%s" % dropout)
    if dropout is None:           # another seed is another mask; the same seed the same bytes
        again = model.forward_train(x.to(DEV), norm="batch", seed=SEED)
        other = model.forward_train(x.to(DEV), norm="batch", seed=SEED + 1)
        assert torch.equal(again, lp) and not torch.equal(other, lp)
        torch.manual_seed(5)
        a = model.forward_train(x.to(DEV), norm="batch")
        torch.manual_seed(5)
        assert torch.equal(a, model.forward_train(x.to(DEV), norm="batch"))
    with pytest.raises(ValueError, match="has no forward_train"):
        model.forward_train(x.to(DEV))


def _gradients(model, cfg, x, label):
    want = {}
    for tag, dtype, rnd in (("exact", F64, lambda t: t), ("yard", torch.float32, ref.round16)):
        params, buffers = _leaves(model, dtype)
        lp, _ = _restate(cfg, params, buffers, x, SEED, dtype, rnd)
        G = _cotangent(lp.shape)
        lp.backward(G.to(dtype))
        want[tag] = {"lp": lp.detach(), **{k: p.grad for k, p in params.items()}}
    lp = model.forward_train(x.to(DEV), norm="batch", seed=SEED)
    assert lp.dtype == torch.float16 and tuple(lp.shape) == (200, 3, 5) and lp.requires_grad
    assert lp.permute(1, 0, 2).is_contiguous()                                   # a view of batch-major rows, as forward(x) returns
    lp.backward(G.to(DEV))
    got = {"lp": lp.detach().cpu(), **{k: p.grad.cpu() for k, p in model.named_parameters()}}
    assert all(p.grad is not None and p.grad.dtype == torch.float32 for p in model.parameters())
    assert not ref.within(got, want["exact"], want["yard"], list(got), label)
    return lp.detach()


def test_running_statistics_after_three_steps_and_inference_on_them():
    model, x = _make()
    cfg = _config()
    batches = [x, (x.float() * 0.5).half(), (x.float() + 0.25).half()]
    before = {k: v.detach().cpu().clone() for k, v in model.named_buffers()}
    model.eval()
    base = model(x.to(DEV)).cpu()                                                # the engine on the fixture's statistics
    model.train()
    with torch.no_grad():
        for i, b in enumerate(batches):
            model.forward_train(b.to(DEV), norm="batch", seed=SEED + i)
    tracked = {}
    for tag, dtype, rnd in (("exact", F64, lambda t: t), ("yard", torch.float32, ref.round16)):
        params, buffers = {k: v.detach().cpu().to(dtype) for k, v in model.named_parameters()}, before
        for i, b in enumerate(batches):
            _, buffers = _restate(cfg, params, buffers, b, SEED + i, dtype, rnd)
        tracked[tag] = buffers
    names = [k for k in before if not k.endswith("num_batches_tracked")]
    got = {k: v.detach().cpu() for k, v in model.named_buffers()}
    assert all(int(got[k]) == int(before[k]) + 3 for k in before if k.endswith("num_batches_tracked"))
    assert not ref.within(got, tracked["exact"], tracked["yard"], names, "three steps")
    model.eval()
    fresh = model(x.to(DEV)).cpu()                                               # load_state_dict / _apply did not run: forward_train does not use the
    params = {k: v.detach().cpu().to(F64) for k, v in model.named_parameters()}  # engine, so the old one answers until it is dropped
    assert torch.equal(fresh, base)
    model._drop_engine()
    fresh = model(x.to(DEV)).cpu()
    new64 = _restate(cfg, params, got, x, 0, F64, training=False)[0]
    old64 = _restate(cfg, params, before, x, 0, F64, training=False)[0]
    d_base, d_new, d_old = ref.dist(base, old64), ref.dist(fresh, new64), ref.dist(fresh, old64)
    print("eval: engine on the fixture's statistics %.3e from its restatement; on the trained ones %.3e, from the old restatement %.3e"
          % (d_base, d_new, d_old))
    assert d_new <= ref.MARGIN * d_base < d_old
    with pytest.raises(ValueError, match="has its BatchNorm in eval mode"):
        model.forward_train(x.to(DEV), norm="batch")


def _chunks(n, seed):
    return tm._batch(n, L=600, seed=seed)


@pytest.mark.parametrize("dropout", [None, 0.0])
def test_twenty_adamw_steps_lower_the_loss(dropout):
    model, _ = _make(dropout)
    x, targets, lengths = _chunks(8, seed=9)
    x = x.to(DEV)
    opt = optim.AdamW([p for p in model.parameters() if p.requires_grad], lr=2e-3)
    torch.manual_seed(3)
    losses = []
    for step in range(21):
        opt.zero_grad(set_to_none=True)
        loss = model.loss(model.forward_train(x, norm="batch"), targets, lengths)["total_loss"]
        losses.append(float(loss.detach()))
        if step < 20:
            opt.scale(loss).backward()
            opt.step(2.0)
    print("quartz_small dropout=%s losses: %s" % (dropout, " ".join("%.4f" % v for v in losses)))
    assert all(v == v and abs(v) != float("inf") for v in losses) and losses[-1] < losses[0]
    assert all(int(b) == 21 for n, b in model.named_buffers() if n.endswith("num_batches_tracked"))


def test_trainer_steps_and_validates():
    model, _ = _make()
    x, targets, lengths = _chunks(8, seed=9)
    batch = (x.float(), targets, lengths)
    with pytest.raises(ValueError, match="has no forward_train without batch statistics"):
        plain = Trainer(model, DEV, [batch], [batch], chunks_per_epoch=8, batch_size=8)
        plain.init_optimizer(2e-3)
        plain.train_one_step(batch)
    trainer = Trainer(model, DEV, [batch], [batch], chunks_per_epoch=8, batch_size=8, grad_accum_split=2, norm="batch")
    trainer.init_optimizer(2e-3)
    before = {k: v.clone() for k, v in model.named_buffers()}
    losses, grad_norm, scale = trainer.train_one_step(batch)
    assert losses["loss"] == losses["loss"] and set(losses) == {"total_loss", "loss", "label_smooth_loss"} and scale > 0
    for name, b in model.named_buffers():
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(before[name]) + 2, name
        else:
            assert not torch.equal(b, before[name]), name
    loss, mean_acc, median_acc = trainer.validate_one_epoch()                     # no decode_batch: the prefix beam search of `evaluate`
    assert loss == loss and 0.0 <= mean_acc <= 100.0 and not model.training


# ---- the command line ---------------------------------------------------------------------------------------------------------------------------
def _write(directory, n, seed):
    import numpy as np
    x, targets, lengths = _chunks(n, seed)
    os.makedirs(directory, exist_ok=True)
    np.save(os.path.join(directory, "chunks.npy"), x[:, 0].float().numpy())
    np.save(os.path.join(directory, "references.npy"), targets.numpy().astype(np.uint8))
    np.save(os.path.join(directory, "reference_lengths.npy"), lengths.numpy().astype(np.uint16))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """data directory, the configuration with every dropout 0 and its uninterrupted two-epoch run (child process)."""
    root = tmp_path_factory.mktemp("train_quartz_cli")
    data = root / "data"
    _write(str(data), 32, seed=21)
    _write(str(data / "validation"), 8, seed=22)
    cfg = root / "cfg.toml"
    with open(cfg, "w") as fh:
        util.dump_toml(_config(0.0), fh)
    out = root / "run"
    done = cli._child("train", out, "--config", cfg, "--directory", data, "--norm", "batch", *COMMON)
    print(done.stdout, done.stderr)
    assert done.returncode == 0, done.stderr + done.stdout
    return dict(root=root, data=data, cfg=cfg, out=out, stdout=done.stdout)


def test_cli_run_trains_and_evaluate_reproduces_its_validation_loss(run):
    out = run["out"]
    config = util.load_toml(out / "config.toml")
    assert config["training"]["norm"] == "batch" and config["model"]["package"] == "bonito.ctc"
    fresh = Model(_config(0.0)).state_dict()
    for epoch, steps in ((1, 4), (2, 8)):
        state = torch.load(out / ("weights_%d.tar" % epoch), map_location="cpu")
        for name in ("encoder.encoder.0.conv.1.running_mean", "encoder.encoder.1.residual.1.running_var", "encoder.encoder.4.conv.1.running_mean"):
            assert bool(torch.isfinite(state[name]).all()) and not torch.equal(state[name], fresh[name]), name
        assert int(state["encoder.encoder.0.conv.1.num_batches_tracked"]) == steps
    with open(out / "training.csv") as fh:
        rows = list(csv.DictReader(fh))
    assert [int(r["epoch"]) for r in rows] == [1, 2]
    done = cli._child("evaluate", out, "--directory", run["data"], "--chunks", "8", "--weights", "2", "--batchsize", "8")
    assert done.returncode == 0, done.stderr
    found = re.search(r"^\* loss mean\s+(\S+)$", done.stdout, flags=re.M)
    print("evaluate: loss mean %s; training.csv: validation_loss %s" % (found.group(1), rows[1]["validation_loss"]))
    # evaluate loads the weights AND the statistics rounded to fp16 (load_model: model.half()), the trainer validates on the fp32
    # masters: the two losses differ by what rounding every parameter to fp16 does, a relative 2^-11 at the most, and by the four
    # printed decimals (measured: 3.3e-6 relative)
    want = float(rows[1]["validation_loss"])
    assert abs(float(found.group(1)) - want) <= 2.0 ** -11 * abs(want) + 5e-5


def test_a_resumed_run_ends_with_the_bytes_of_the_uninterrupted_one(run, capsys):
    """With dropout 0: the dropout seeds come from torch's generator, whose state no checkpoint holds (the reference's neither)."""
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
        for key in a:
            if isinstance(a[key], torch.Tensor):
                assert a[key].dtype == b[key].dtype and a[key].numpy().tobytes() == b[key].numpy().tobytes(), (name, key)


def test_train_without_norm_is_refused_with_an_empty_directory(run, capsys):
    for extra in (["--config", str(run["cfg"])], ["--pretrained", str(run["out"])]):
        refused = run["root"] / ("refused_%s" % extra[0].strip("-"))
        with pytest.raises(SystemExit) as exc:
            main(["train", str(refused)] + extra + ["--directory", str(run["data"])] + COMMON)
        assert exc.value.code == 1 and "has no forward_train" in capsys.readouterr().out and os.listdir(refused) == []
    out = run["root"] / "finetuned"                                                 # --pretrained <ctc dir> --norm batch with no further option
    assert main(["train", str(out), "--pretrained", str(run["out"]), "--directory", str(run["data"]), "--norm", "batch", "--epochs", "1"]
                + COMMON[2:]) == 0
    state = torch.load(out / "weights_1.tar", map_location="cpu")
    assert int(state["encoder.encoder.0.conv.1.num_batches_tracked"]) == 8 + 4

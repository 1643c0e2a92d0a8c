"""SeqdistModel.forward_train for the transformer family on the device (-m gpu): a small v5-style model (tests/transformer_train_ref.py:
model_config - convs 1 -> 16 -> 32 -> 128, permute [0,2,1], two encoder layers with d_model 128, 2 heads, dim_feedforward 256 and
window (3, 5), upsample x2, linear CRF head with scale 5 and clamp +-5) on chunks of 240 samples: forward_train -> loss -> backward
against a torch restatement of the encoder, optim.AdamW steps, and ``python -m bonito_amd train`` / ``evaluate``.

With the upstream gradient d loss / d scores captured by a hook and the clamp's mask read from the stored scores, exact = fp64 autograd
through the restatement and yardstick = the same in fp16 on the CPU; every parameter's gradient must satisfy
dist(kernel) <= 2 dist(yardstick), the project's margin for composed training layers."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import conftest
import test_train_layers_ref_cpu as lstm_family
import transformer_train_ref as ref
from bonito_amd import optim, util
from bonito_amd.crf.model import Model as CrfModel
from bonito_amd.transformer import Model

pytestmark = pytest.mark.gpu

DEV = "cuda"
PARITY = 2.1e-2         # tests/test_gpu_train_model.py's value: the tolerance between engine paths (max |score difference|)
M = ref.MODEL
L, T_OUT, N_SCORES = 240, 160, 256


def _model(seed):
    torch.manual_seed(seed)
    model = Model(ref.model_config())
    with torch.no_grad():                     # fp16-representable master weights: the restatement and the layers see the same values
        for p in model.parameters():
            p.copy_(p.half().float())
    return model.to(DEV)


@functools.lru_cache(maxsize=None)
def _run():
    """One forward_train -> loss -> backward on three chunks, and the captured upstream gradient."""
    model = _model(0)
    x, targets, lengths = ref.model_batch(3)
    captured = []
    scores = model.forward_train(x.to(DEV))
    scores.register_hook(captured.append)
    loss = model.loss(scores, targets, lengths)
    loss.backward()
    torch.cuda.synchronize()
    return model, x, scores.detach(), float(loss.detach()), captured[0].detach()


def test_forward_train_has_the_shape_layout_and_values_of_forward():
    model, x, scores, loss, dscores = _run()
    assert loss == loss and abs(loss) != float("inf")
    assert model._hip is None                                  # forward_train builds no engine
    want = model(x.to(DEV))
    assert scores.shape == want.shape == (3, T_OUT, N_SCORES) and scores.dtype == want.dtype == torch.float16
    assert scores.is_contiguous() and want.is_contiguous() and scores.stride() == want.stride()
    assert float(scores.abs().max()) <= M["clamp"][1]
    diff = float((scores.float() - want.float()).abs().max())
    print("forward_train against forward: max |difference| = %.3e" % diff)
    assert diff < PARITY
    assert dscores.shape == scores.shape


def test_every_trainable_parameter_receives_a_gradient():
    model = _run()[0]
    names = [name for name, p in model.named_parameters()]
    assert len(names) == 3 * 2 + M["depth"] * len(ref.LAYER_PARAMS) + 2 + 1
    for name, p in model.named_parameters():
        assert p.requires_grad and p.grad is not None and p.grad.dtype == torch.float32 and p.grad.shape == p.shape, name
        assert bool(torch.isfinite(p.grad).all()) and int(torch.count_nonzero(p.grad)) > 0, name
    for layer in model.encoder.transformer_encoder:
        assert layer.deepnorm_alpha.grad is None


def test_every_parameter_gradient_is_within_twice_the_yardstick():
    model, x, scores, loss, dscores = _run()
    params = {name: p.detach().cpu() for name, p in model.encoder.named_parameters()}
    mask = ((scores > M["clamp"][0]) & (scores < M["clamp"][1])).cpu()
    kw = dict(convs=M["convs"], depth=M["depth"], nhead=M["nhead"], window=M["window"], alpha=float(model.encoder.transformer_encoder[0].deepnorm_alpha),
              upsample=M["upsample"], scale=M["scale"], clamp=M["clamp"])
    y64, exact = ref.model_torch(params, x[:, 0], dscores.cpu(), mask, dtype=torch.float64, **kw)
    _, yard = ref.model_torch(params, x[:, 0], dscores.cpu(), mask, dtype=torch.float16, **kw)
    assert sorted(exact) == sorted(params)
    print("clamped scores: %d of %d; dist(scores) = %.3e" % (int((~mask).sum()), mask.numel(), ref.dist(scores, y64)))
    assert ref.dist(scores, y64) < 1e-2
    failed = []
    for name, p in model.encoder.named_parameters():
        dk, dy = ref.dist(p.grad, exact[name]), ref.dist(yard[name], exact[name])
        print("chain %-50s: dist(kernel) = %.3e  dist(yardstick) = %.3e  ratio = %.3f" % (name, dk, dy, dk / dy))
        if not dk <= ref.MARGIN * dy:
            failed.append((name, dk, dy))
    assert not failed, failed


def test_twenty_steps_of_adamw_lower_the_loss():
    model = _model(2)
    x, targets, lengths = ref.model_batch(8, seed=9)
    x = x.to(DEV)
    opt = optim.AdamW(model.parameters(), lr=1e-3, loss_scale=4096.0)
    losses, skipped = [], 0
    for step in range(21):
        opt.zero_grad(set_to_none=True)
        loss = model.loss(model.forward_train(x), targets, lengths)
        losses.append(float(loss.detach()))
        assert losses[-1] == losses[-1] and abs(losses[-1]) != float("inf"), losses
        if step == 20:
            break
        opt.scale(loss).backward()
        opt.step(max_norm=2.0)
        skipped += int(opt.last()[2])
    print("losses:", " ".join("%.4f" % v for v in losses), "skipped steps:", skipped)
    assert losses[-1] < losses[0]
    assert model._hip is None


def _write_chunks(directory, n, seed):
    x, targets, lengths = ref.model_batch(n, seed=seed)
    os.makedirs(directory, exist_ok=True)
    np.save(os.path.join(directory, "chunks.npy"), x[:, 0].float().numpy())
    np.save(os.path.join(directory, "references.npy"), targets.numpy().astype(np.uint8))
    np.save(os.path.join(directory, "reference_lengths.npy"), lengths.numpy().astype(np.uint16))


def _child(*argv):
    env = dict(os.environ, PYTHONPATH=conftest.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "bonito_amd"] + [str(a) for a in argv], cwd=conftest.ROOT, env=env, capture_output=True,
                          text=True, timeout=300)


def test_cli_train_writes_a_directory_whose_loss_evaluate_reproduces(tmp_path):
    """The epoch line's validation loss is the engine's on the fp32 master weights; ``evaluate`` loads the directory with load_model's
    half = True. For the LSTM family that changes nothing (tests/test_gpu_train_cli.py: 1e-3 on figures printed with four decimals). A
    transformer layer's norm gains, its out_proj bias and deepnorm_alpha are read by the engine as fp32, so the fp16 checkpoint rounds
    them: 2^-11 relative each (deepnorm_alpha 1.4142136 -> 1.4140625). The scores are linear read-outs of RMS-normalised activations,
    so the loss moves by that relative order; twice it, 2^-10 of the loss, is allowed beside the 1e-3."""
    data, cfg, out = tmp_path / "data", tmp_path / "cfg.toml", tmp_path / "run"
    _write_chunks(str(data), 16, seed=21)
    _write_chunks(str(data / "validation"), 8, seed=22)
    with open(cfg, "w") as fh:
        util.dump_toml(ref.model_config(), fh)
    done = _child("train", out, "--config", cfg, "--directory", data, "--epochs", "1", "--batch", "8", "--chunks", "16", "--valid-chunks", "8")
    print(done.stdout, done.stderr)
    assert done.returncode == 0, done.stderr
    assert {"config.toml", "training.csv", "weights_1.tar", "losses_1.csv"} <= set(os.listdir(out))
    assert util.load_toml(out / "config.toml")["model"]["encoder"] == ref.model_config()["model"]["encoder"]
    lines = re.findall(r"^\[epoch (\d)\] directory=\S+ loss=(\S+) mean_acc=(\S+)% median_acc=(\S+)%$", done.stdout, flags=re.M)
    assert [int(m[0]) for m in lines] == [1]
    model = util.load_model(str(out), DEV)
    assert model(ref.model_batch(8, seed=22)[0].to(DEV)).shape == (8, T_OUT, N_SCORES)
    done = _child("evaluate", out, "--directory", data, "--chunks", "8", "--weights", "1", "--batchsize", "8")
    assert done.returncode == 0, done.stderr
    found = re.search(r"^\* loss mean\s+(\S+)$", done.stdout, flags=re.M)
    got, want = float(found.group(1)), float(lines[0][1])
    print("evaluate: loss mean %s; the epoch line: loss=%s; difference / loss = %.3e" % (found.group(1), lines[0][1], abs(got - want) / want))
    assert abs(got - want) <= 1e-3 + 2.0 ** -10 * want


def test_the_pinned_refusals_hold_on_the_device():
    x = ref.model_batch(2)[0].to(DEV)
    refused = Model(ref.model_config(norm="batchnorm")).to(DEV)
    with pytest.raises(ValueError, match=r"layer 0 \(Convolution\) carries a norm \(batchnorm\)"):
        refused.forward_train(x)
    assert refused._hip is None
    lstm = CrfModel(lstm_family._config(kind="upsample")).to(DEV)           # the upsample after time-major activations
    with pytest.raises(ValueError, match=r"layer 9 \(LinearUpsample\) has no training forward"):
        lstm.forward_train(x[:, :, :120])
    assert lstm._hip is None
    with pytest.raises(ValueError, match="holds float16 parameters"):
        Model(ref.model_config()).to(DEV).half().forward_train(x)

"""``python -m bonito_amd train`` and bonito_amd.training.Trainer on the device (-m gpu): the 32-feature old-style model of
tests/test_gpu_train_model.py on 40 synthetic chunks of 120 samples (its `_batch` recipe: 32 to train on, 8 in validation/).

The run the other tests compare against is made once, in a child process; the resumed run and the refusals call the same ``main``
in this process."""
import csv
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import conftest
import test_gpu_train_model as tm
from bonito_amd import util
from bonito_amd.__main__ import main
from bonito_amd.crf.model import Model
from bonito_amd.training import Trainer

pytestmark = pytest.mark.gpu

DEV = "cuda"
GOLD = json.load(open(os.path.join(conftest.GOLDEN, "schedule_cases.json")))
COMMON = ["--epochs", "2", "--batch", "8", "--chunks", "32", "--valid-chunks", "8", "--save-optim-every", "1"]


def _write_chunks(directory, n, seed):
    x, targets, lengths = tm._batch(n, seed=seed)
    os.makedirs(directory, exist_ok=True)
    np.save(os.path.join(directory, "chunks.npy"), x[:, 0].float().numpy())
    np.save(os.path.join(directory, "references.npy"), targets.numpy().astype(np.uint8))
    np.save(os.path.join(directory, "reference_lengths.npy"), lengths.numpy().astype(np.uint16))


def _child(*argv):
    env = dict(os.environ, PYTHONPATH=conftest.ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run([sys.executable, "-m", "bonito_amd"] + [str(a) for a in argv], cwd=conftest.ROOT, env=env, capture_output=True,
                          text=True, timeout=300)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """data directory, config file and the uninterrupted two-epoch run (child process)."""
    root = tmp_path_factory.mktemp("train_cli")
    data = root / "data"
    _write_chunks(str(data), 32, seed=21)
    _write_chunks(str(data / "validation"), 8, seed=22)
    cfg = root / "cfg.toml"
    with open(cfg, "w") as fh:
        util.dump_toml({"model": {"package": "bonito_amd.crf"}, **tm.OLD}, fh)
    out = root / "run"
    done = _child("train", out, "--config", cfg, "--directory", data, *COMMON)
    print(done.stdout, done.stderr)
    assert done.returncode == 0, done.stderr
    return dict(root=root, data=data, cfg=cfg, out=out, stdout=done.stdout)


def _rows(path):
    with open(path, newline="") as fh:
        return list(csv.DictReader(fh))


def test_trainer_lowers_the_loss_on_one_fixed_batch():
    torch.manual_seed(2)
    model = Model(tm.OLD)
    x, targets, lengths = tm._batch(8, seed=9)
    batch = (x.float(), targets, lengths)
    trainer = Trainer(model, DEV, [batch], [batch], chunks_per_epoch=8, batch_size=8,
                      lr_scheduler_fn=lambda opt, steps, epochs, last: torch.optim.lr_scheduler.LambdaLR(opt, lambda step: 1.0))
    trainer.init_optimizer(2e-3)
    sched = trainer.get_lr_scheduler(1)
    losses, scales, norms = [], [], []
    for step in range(60):
        step_losses, grad_norm, scale = trainer.train_one_step(batch)
        sched.step()
        losses.append(step_losses["loss"])
        scales.append(scale)
        norms.append(grad_norm)
    below = next((i for i, v in enumerate(losses) if v < losses[0]), None)
    print("losses:", " ".join("%.4f" % v for v in losses))
    print("scales:", sorted(set(scales)), "skipped steps:", sum(not math.isfinite(n) for n in norms), "first step below the first loss:", below)
    assert all(math.isfinite(v) for v in losses) and min(scales) > 0 and trainer.optimizer.control()["scale"] > 0
    assert losses[-1] < losses[0]
    assert model._hip is None                                    # training builds no engine


def test_cli_run_writes_a_directory_that_loads_and_evaluates(run):
    out = run["out"]
    names = sorted(os.listdir(out))
    assert names == sorted(["config.toml", "training.csv"] + ["%s_%d.%s" % (n, e, x) for n, x in (("weights", "tar"), ("optim", "tar"), ("losses", "csv"))
                                                              for e in (1, 2)])
    lrs = []
    for epoch in (1, 2):
        rows = _rows(out / ("losses_%d.csv" % epoch))
        assert list(rows[0]) == ["chunks", "time", "grad_norm", "lr", "scale", "loss"] and [int(r["chunks"]) for r in rows] == [8, 16, 24, 32]
        for r in rows:
            print("epoch %d: %s" % (epoch, dict(r)))
            assert math.isfinite(float(r["grad_norm"])) and float(r["scale"]) > 0 and math.isfinite(float(r["loss"]))
        lrs += [float(r["lr"]) for r in rows]
    assert lrs == GOLD["schedules"][0]
    log = _rows(out / "training.csv")
    assert [int(r["epoch"]) for r in log] == [1, 2] and list(log[0]) == ["time", "duration", "epoch", "train_loss", "validation_loss", "validation_mean",
                                                                        "validation_median"]
    config = util.load_toml(out / "config.toml")
    assert config["encoder"] == tm.OLD["encoder"] and config["training"]["batch"] == 8 and config["training"]["lr"] == "2e-3"
    lines = re.findall(r"^\[epoch (\d)\] directory=\S+ loss=(\S+) mean_acc=(\S+)% median_acc=(\S+)%$", run["stdout"], flags=re.M)
    assert [int(m[0]) for m in lines] == [1, 2]
    assert abs(float(lines[1][1]) - float(log[1]["validation_loss"])) < 1e-4
    model = util.load_model(str(out), DEV)
    assert model(tm._batch(8, seed=22)[0].to(DEV)).shape == (8, 24, 256)
    done = _child("evaluate", out, "--directory", run["data"], "--chunks", "8", "--weights", "2", "--batchsize", "8")
    assert done.returncode == 0, done.stderr
    found = re.search(r"^\* loss mean\s+(\S+)$", done.stdout, flags=re.M)
    print("evaluate: loss mean %s; the epoch line: loss=%s" % (found.group(1), lines[1][1]))
    assert abs(float(found.group(1)) - float(lines[1][1])) <= 1e-3


def test_a_resumed_run_ends_with_the_bytes_of_the_uninterrupted_one(run, capsys):
    out = run["root"] / "resumed"
    base = ["train", str(out), "--config", str(run["cfg"]), "--directory", str(run["data"])]
    one = [a if a != "2" else "1" for a in COMMON[:2]] + COMMON[2:]
    assert main(base + one) == 0
    with pytest.raises(SystemExit) as exc:
        main(base + COMMON)
    assert exc.value.code == 1 and "[error] %s exists, use -f to force continue training." % out in capsys.readouterr().out
    assert main(base + COMMON + ["-f", "--restore-optim"]) == 0
    assert "[picking up weights, optim state from epoch 1]" in capsys.readouterr().out

    def flat(obj, prefix=""):
        if isinstance(obj, torch.Tensor):
            return {prefix: obj}
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
                assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape and a[key].numpy().tobytes() == b[key].numpy().tobytes(), (name, key)
            elif not key.endswith(("initial_lr", "/lr")):          # the scheduler's bookkeeping; the learning rates applied are in losses_2.csv
                assert a[key] == b[key], (name, key)
    assert [r["lr"] for r in _rows(out / "losses_2.csv")] == [r["lr"] for r in _rows(run["out"] / "losses_2.csv")]


def test_no_amp_and_a_model_without_forward_train_are_refused_before_any_file(run, capsys):
    out = run["root"] / "refused"
    with pytest.raises(SystemExit) as exc:
        main(["train", str(out), "--config", str(run["cfg"]), "--directory", str(run["data"]), "--no-amp"] + COMMON)
    assert exc.value.code == 1 and "--no-amp is not served" in capsys.readouterr().out and os.listdir(out) == []
    quartz = run["root"] / "quartz.toml"
    with open(quartz, "w") as fh:
        util.dump_toml(conftest.load_ctc_fixture()[0], fh)
    out = run["root"] / "refused_quartz"
    with pytest.raises(SystemExit) as exc:
        main(["train", str(out), "--config", str(quartz), "--directory", str(run["data"])] + COMMON)
    assert exc.value.code == 1 and "has no forward_train" in capsys.readouterr().out and os.listdir(out) == []
    norm = run["root"] / "norm.toml"                             # a model forward_train refuses: its message, in front of any file
    with open(norm, "w") as fh:
        util.dump_toml({"model": {"package": "bonito_amd.crf"}, **tm._new_config(norm="batchnorm")}, fh)
    out = run["root"] / "refused_norm"
    with pytest.raises(SystemExit) as exc:
        main(["train", str(out), "--config", str(norm), "--directory", str(run["data"])] + COMMON)
    assert exc.value.code == 1 and "carries a norm (batchnorm)" in capsys.readouterr().out and os.listdir(out) == []

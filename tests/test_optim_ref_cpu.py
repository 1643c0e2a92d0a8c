"""The definition of the optimizer step (tests/optim_ref.py) against torch on the CPU, and the host side of training: schedules, the
quantile clip and the data split against values recorded from the reference (tests/golden/schedule_cases.json), the TOML writer, the
checkpoint choice, every refusal, and the C entries' argument checks. No GPU."""
import copy
import ctypes as C
import io
import json
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import optim_ref as ref
import train_cases
from conftest import GOLDEN, ROOT
from bonito_amd import _lib, data, optim, schedule, training, util
from bonito_amd.nn import NoTorchCompute

GOLD = json.load(open(os.path.join(GOLDEN, "schedule_cases.json")))
SIZES = (7, 33, 5)


def _problem(steps=5, seed=0):
    rng = np.random.default_rng(seed)
    params = [rng.standard_normal(n) for n in SIZES]
    grads = [[rng.standard_normal(n) * 0.7 for n in SIZES] for _ in range(steps)]
    return params, grads


def _torch_run(params, grads, lr, max_norm, weight_decay, betas=(0.9, 0.999), eps=1e-8):
    ps = [torch.nn.Parameter(torch.tensor(p, dtype=torch.float64)) for p in params]
    opt = torch.optim.AdamW(ps, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)
    norms = []
    for step in grads:
        for p, g in zip(ps, step):
            p.grad = torch.tensor(g, dtype=torch.float64)
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm)))
        opt.step()
    return [p.detach().numpy() for p in ps], [opt.state[p]["exp_avg"].numpy() for p in ps], [opt.state[p]["exp_avg_sq"].numpy() for p in ps], norms


def _ref_run(params, grads, lr, max_norm, weight_decay, loss_scale=1024.0, defect=None, betas=(0.9, 0.999), eps=1e-8):
    ps, ms, vs = list(params), [np.zeros(n) for n in SIZES], [np.zeros(n) for n in SIZES]
    ctl, norms = ref.new_control(loss_scale), []
    for step in grads:
        ps, ms, vs, ctl = ref.step_fp64(ps, [g * loss_scale for g in step], ms, vs, ctl, lr, max_norm, betas, eps, weight_decay, defect=defect)
        norms.append(ctl["grad_norm"])
    return ps, ms, vs, norms, ctl


def _worst(a, b):
    return max(float(np.max(np.abs(x - y) / (np.abs(y) + 1e-300))) for x, y in zip(a, b))


CONFIGS = [dict(lr=2e-3, max_norm=None, weight_decay=0.0), dict(lr=2e-3, max_norm=None, weight_decay=0.01),
           dict(lr=2e-3, max_norm=1.5, weight_decay=0.0), dict(lr=5e-2, max_norm=1.5, weight_decay=0.1), dict(lr=2e-3, max_norm=1e3, weight_decay=0.01)]
# fp64 rounding: torch orders the operations differently (lerp, addcdiv, step_size folded into the quotient), a few roundings per step
FP64_TOL = 1e-12


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "lr%g_clip%s_wd%g" % (c["lr"], c["max_norm"], c["weight_decay"]))
def test_fp64_restatement_agrees_with_torch_adamw_and_clip_grad_norm(cfg):
    params, grads = _problem()
    tp, tm, tv, tnorms = _torch_run(params, grads, **cfg)
    rp, rm, rv, rnorms, ctl = _ref_run(params, grads, **cfg)
    assert ctl["step"] == 5 and ctl["beta1_pow"] == optim.beta_power(0.9, 5)
    for name, got, want in (("p", rp, tp), ("m", rm, tm), ("v", rv, tv)):
        worst = _worst(got, want)
        print("%s: largest relative difference from torch %.3e" % (name, worst))
        assert worst < FP64_TOL, name
    if cfg["max_norm"] is not None:
        assert np.allclose(rnorms, tnorms, rtol=1e-14, atol=0)
        assert all((n > cfg["max_norm"]) == (cfg["max_norm"] == 1.5) for n in rnorms)      # the clip is active in the cases meant to have it so


@pytest.mark.parametrize("defect", [d for d in ref.DEFECTS if d != "step_on_skip"])
def test_a_planted_defect_is_rejected_by_the_comparison_with_torch(defect):
    cfg = dict(lr=5e-2, max_norm=1.5, weight_decay=0.1)
    params, grads = _problem()
    if defect == "clip_without_1e-6":               # gradients small enough for the 1e-6 to matter: norm of order 1e-4
        grads = [[g * 1e-4 for g in step] for step in grads]
        cfg["max_norm"] = 1e-5
    if defect == "eps_inside_sqrt":                 # gradients of the size of eps
        grads = [[g * 1e-8 for g in step] for step in grads]
        cfg["max_norm"] = None
    tp, tm, tv, _ = _torch_run(params, grads, **cfg)
    good = _ref_run(params, grads, **cfg)
    assert max(_worst(good[0], tp), _worst(good[1], tm), _worst(good[2], tv)) < FP64_TOL
    bad = _ref_run(params, grads, defect=defect, **cfg)
    worst = max(_worst(bad[0], tp), _worst(bad[1], tm), _worst(bad[2], tv))
    print("%s: largest relative difference from torch %.3e" % (defect, worst))
    assert worst > 1e3 * FP64_TOL


def test_loss_scale_rule_on_a_hand_written_sequence():
    """skip, skip, then growth_interval clean steps: the scale halves twice and doubles once; a skip advances nothing else."""
    interval = 3
    kw = dict(max_norm=2.0, growth_interval=interval)
    c = ref.new_control(65536.0)
    c = ref.finalise(c, float("inf"), **kw)
    assert (c["scale"], c["growth_tracker"], c["step"], c["beta1_pow"], c["skipped"], c["scale_used"]) == (32768.0, 0, 0, 1.0, 1, 65536.0)
    c = ref.finalise(c, float("nan"), **kw)
    assert (c["scale"], c["growth_tracker"], c["step"], c["beta2_pow"], c["skipped"]) == (16384.0, 0, 0, 1.0, 1)
    for k in range(interval):
        c = ref.finalise(c, (16384.0 * 3.0) ** 2, **kw)
        assert c["skipped"] == 0 and c["step"] == k + 1 and c["grad_norm"] == 3.0 and c["scale_used"] == 16384.0 * (1 if k < interval else 2)
        assert c["clip_coef"] == 2.0 / (3.0 + 1e-6) and c["grad_mul"] == c["clip_coef"] / 16384.0
        assert (c["scale"], c["growth_tracker"]) == ((16384.0, k + 1) if k + 1 < interval else (32768.0, 0))
    assert c["beta1_pow"] == 0.9 * 0.9 * 0.9 and c["bias1"] == 1.0 - 0.9 * 0.9 * 0.9 and c["bias2_sqrt"] == math.sqrt(1.0 - 0.999 * 0.999 * 0.999)
    fixed = ref.finalise(ref.new_control(65536.0), float("inf"), use_scale=False, **kw)     # a disabled scale is 1 and a bad sum still skips
    assert fixed["skipped"] == 1 and fixed["scale_used"] == 1.0 and fixed["scale"] == 65536.0
    # the planted defect: a skipped call that advances the step
    bad = ref.finalise(ref.new_control(65536.0), float("inf"), defect="step_on_skip", **kw)
    assert bad["step"] == 1 and bad["beta1_pow"] == 0.9


def test_fp32_restatement_stays_near_the_fp64_one_and_leaves_its_inputs():
    rng = np.random.default_rng(3)
    p, g, m, v = (rng.standard_normal(1000).astype(np.float32) for _ in range(4))
    v = np.abs(v)
    kept = [a.copy() for a in (p, g, m, v)]
    ctl = ref.finalise(ref.new_control(1024.0), ref.sum_of_squares([g]), 2.0)
    got = ref.adamw_fp32(p, g, m, v, ctl, 2e-3)
    want = ref.adamw_fp64(p, g, m, v, ctl, 2e-3)
    for a, b in zip(got, want):
        assert a.dtype == np.float32 and np.allclose(a, b, rtol=1e-5, atol=1e-7)
    assert all(np.array_equal(a, b) for a, b in zip((p, g, m, v), kept))
    skipped = ref.finalise(ref.new_control(1024.0), float("inf"), 2.0)
    assert all(np.array_equal(a, b) for a, b in zip(ref.adamw_fp32(p, g, m, v, skipped, 2e-3), (p, m, v)))
    with np.errstate(over="ignore"):
        assert ref.sum_of_squares([np.array([3e19], np.float32)]) == float("inf") and math.isnan(ref.sum_of_squares([np.array([np.nan], np.float32)]))
    assert ref.ulp_distance(np.float32([1.0, -1.0]), np.float32([np.nextafter(np.float32(1), np.float32(2)), -1.0])) == 1


# ---- schedules, the quantile clip, the data split: the reference's values -------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(train_cases.SCHEDULES)))
def test_schedules_give_the_learning_rates_of_the_reference(i):
    name, kwargs, lr, steps_per_epoch, epochs, last_epoch = train_cases.SCHEDULES[i]
    optimizer = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)
    sched = getattr(schedule, name)(**kwargs)(optimizer, steps_per_epoch, epochs, last_epoch)
    lrs = []
    for _ in range((epochs - last_epoch) * steps_per_epoch):
        lrs.append(float(sched.get_last_lr()[0]))
        optimizer.step()
        sched.step()
    assert lrs == GOLD["schedules"][i]


def test_schedule_pieces_and_the_quantile_clip():
    piece = schedule.piecewise_schedule([0.25, 0.5], [schedule.linear_schedule(0.0, 1.0), schedule.const_schedule(1.0),
                                                      schedule.cosine_decay_schedule(1.0, 0.1)])
    assert [float(piece(t)) for t in GOLD["piecewise"]["t"]] == GOLD["piecewise"]["y"]
    assert [float(schedule.inverse_sqrt_decay_schedule(3.0)(t)) for t in GOLD["piecewise"]["t"]] == GOLD["inverse_sqrt"]
    clip, got = training.ClipGrad(), []
    assert clip.max_norm() == 2e6
    for norm in train_cases.CLIP_NORMS:
        got.append(clip.max_norm())
        clip.append(norm)
    assert got == GOLD["clip_max_norms"] and min(got) < 10 and not np.isnan(clip.buffer).any()


@pytest.mark.parametrize("name", list(train_cases.DATA))
def test_load_numpy_splits_as_the_reference_does(name, tmp_path):
    limit, valid_chunks = train_cases.write_data_case(str(tmp_path), name)
    loaded = dict(zip(("train", "valid"), data.load_numpy(limit, str(tmp_path), valid_chunks=valid_chunks)))
    for key, (chunks, targets, lengths) in loaded.items():
        want = GOLD["data"][name][key]
        assert [int(v) for v in lengths] == want["ids"], key
        assert [len(chunks), 1, chunks.shape[1]] == want["chunks_shape"] and list(targets.shape) == want["targets_shape"], key


def test_batches_are_index_slices_in_an_order_the_seed_and_epoch_fix(tmp_path):
    train_cases.write_chunks(str(tmp_path), 21)
    train, valid = data.load_data(tmp_path, 0, 5, batch_size=8, seed=25)
    assert len(train) == 2 and len(valid) == 1 and len(train.lengths) == 16
    train.set_epoch(2)
    first = [b[2].tolist() for b in train]
    assert [b[2].tolist() for b in train] == first                                     # the same epoch again: the same batches
    assert sum(first, []) == np.random.default_rng([25, 2]).permutation(16).tolist()
    train.set_epoch(3)
    assert [b[2].tolist() for b in train] != first
    x, t, n = next(iter(valid))
    assert x.shape == (5, 1, 12) and x.dtype == torch.float32 and t.dtype == n.dtype == torch.int64 and n.tolist() == [16, 17, 18, 19, 20]
    empty = tmp_path / "script"
    empty.mkdir()
    (empty / "dataset.py").write_text("")
    with pytest.raises(IOError, match="dataset.py loader is not supported"):
        data.load_data(empty, 0, None, 8, 0)
    with pytest.raises(IOError, match="no chunks.npy"):
        data.load_data(tmp_path / "nothing", 0, None, 8, 0)
    from bonito_amd.cli import evaluate
    assert evaluate.load_numpy_datasets is data.load_numpy_datasets and evaluate.decode_ref is util.decode_ref


# ---- host pieces ------------------------------------------------------------------------------------------------------------------------
def test_dump_toml_round_trips_the_training_configs(tmp_path):
    import test_gpu_train_model as tm
    extra = {"training": {"lr": "2e-3", "directory": tmp_path, "force": False, "valid_chunks": None, "seed": 25, "pwd": 'a "quoted"\\path\n'},
             "model": {"package": "bonito_amd.crf"}, "optim": {"betas": [0.9, 0.999], "eps": 1e-08, "big": 1e22, "neg": -0.5, "whole": 3.0},
             "odd key": {"a.b": 1}, "mixed": [{"x": 1}, 2]}
    for config in (tm.OLD, tm._new_config()):
        full = {**config, **extra}
        path = tmp_path / "config.toml"
        with open(path, "w") as fh:
            util.dump_toml(full, fh)
        back = util.load_toml(path)
        want = json.loads(json.dumps(full, default=str))
        del want["training"]["valid_chunks"]                   # TOML has no null: the key is left out
        assert back == want
        assert type(back["optim"]["whole"]) is float and type(back["training"]["seed"]) is int and back["training"]["force"] is False
    with pytest.raises(TypeError, match="no TOML form"):
        util.dump_toml({"a": {"b": object()}})


def test_load_state_chooses_the_epoch(tmp_path, capsys):
    model = torch.nn.Linear(3, 2)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    assert training.load_state(str(tmp_path), "cpu", model, opt) == 0 and training.load_state(str(tmp_path), "cpu", model) == 0
    model(torch.ones(1, 3)).sum().backward()
    opt.step()
    for n in (1, 3, 12):
        with torch.no_grad():
            model.bias.fill_(float(n))
        torch.save(model.state_dict(), tmp_path / ("weights_%d.tar" % n))
    for n in (1, 2, 3):
        opt.param_groups[0]["lr"] = n * 1e-3
        torch.save(opt.state_dict(), tmp_path / ("optim_%d.tar" % n))
    (tmp_path / "weights_x.tar").write_text("not a checkpoint")
    assert training.load_state(str(tmp_path), "cpu", model) == 12 and float(model.bias.data[0]) == 12.0          # the newest weights
    assert "[picking up weights state from epoch 12]" in capsys.readouterr().out
    assert training.load_state(str(tmp_path), "cpu", model, opt) == 3 and float(model.bias.data[0]) == 3.0      # the newest with both files
    assert opt.param_groups[0]["lr"] == 3e-3
    assert "[picking up weights, optim state from epoch 3]" in capsys.readouterr().out


def test_csv_logger_appends_under_the_header_it_finds(tmp_path):
    from bonito_amd.io import CSVLogger
    path = tmp_path / "losses_1.csv"
    with CSVLogger(path) as log:
        log.append({"chunks": 8, "loss": 1.5})
        with pytest.raises(ValueError, match="set already"):
            log.set_columns(["a"])
    with CSVLogger(path) as log:
        log.append({"loss": 1.25, "extra": 3})
    assert path.read_text().splitlines() == ["chunks,loss", "8,1.5", "-,1.25"]


def test_refusals_of_the_optimizer():
    with pytest.raises(NoTorchCompute, match="runs on a HIP device only"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(3))])
    with pytest.raises(ValueError, match="must be float32"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(3, dtype=torch.float16))])
    with pytest.raises(ValueError, match="not contiguous"):
        optim.AdamW([torch.nn.Parameter(torch.zeros(3, 4).t())])
    for kw, text in ((dict(lr=-1.0), "lr"), (dict(eps=-1e-8), "eps"), (dict(betas=(1.0, 0.9)), "betas"), (dict(weight_decay=-0.1), "weight_decay"),
                     (dict(loss_scale=0.0), "loss_scale"), (dict(growth_interval=0), "growth_interval")):
        with pytest.raises(ValueError, match=text):
            optim.AdamW([torch.nn.Parameter(torch.zeros(3))], **kw)


def test_refusals_of_the_trainer_and_the_command_line(tmp_path, capsys):
    model = types.SimpleNamespace(forward_train=None, loss=None, to=lambda device: model)
    with pytest.raises(ValueError, match="use_amp=False is not served"):
        training.Trainer(model, "cpu", [], [], use_amp=False, chunks_per_epoch=8, batch_size=8)
    with pytest.raises(ValueError, match="has no forward_train"):
        training.Trainer(torch.nn.Linear(2, 2), "cpu", [], [], chunks_per_epoch=8, batch_size=8)
    from bonito_amd.__main__ import main
    existing = tmp_path / "run"
    existing.mkdir()
    with pytest.raises(SystemExit) as exc:
        main(["train", str(existing), "--config", "x.toml", "--directory", str(tmp_path)])
    assert exc.value.code == 1 and "[error] %s exists, use -f to force continue training." % existing in capsys.readouterr().out
    fresh = tmp_path / "fresh"
    with pytest.raises(SystemExit) as exc:
        main(["train", str(fresh), "--config", "x.toml", "--directory", str(tmp_path), "--no-amp"])
    assert exc.value.code == 1 and "--no-amp is not served" in capsys.readouterr().out
    assert fresh.is_dir() and list(fresh.iterdir()) == []


# ---- the C entries ----------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_bound_and_exported_and_the_enum_matches():
    header = open(os.path.join(ROOT, "include", "bonito_hip.h")).read()
    handle = _lib.lib()
    for name in ("bh_optim_chunk", "bh_optim_workspace", "bh_optim_norm", "bh_optim_update", "bh_optim_last_kernel"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.SIGNATURES and hasattr(handle, name), name
    enum = header[header.index("enum bh_optim_ctl {"):]
    table = {k.lower(): int(v) for k, v in re.findall(r"BH_OPTIM_(\w+)\s*=\s*(\d+)", enum[:enum.index("};")])}
    assert table.pop("ctl_words") == optim.CTL_WORDS and table == optim.CTL
    assert handle.bh_optim_chunk() == int(re.search(r"#define BH_OPTIM_CHUNK (\d+)", header).group(1)) == 8192
    assert handle.bh_abi_version() == 1
    assert "optim.hip" in open(os.path.join(ROOT, "build.py")).read().split("EXTRA_FLAGS = ")[1].splitlines()[0]


def test_argument_errors_come_back_before_any_launch():
    """Every pointer below is a made-up address that no kernel may read: each call is refused by the argument checks."""
    handle = _lib.lib()
    chunk = handle.bh_optim_chunk()
    p = C.c_void_p(4096)
    ptrs = (C.c_void_p * 2)(4096, 8192)
    sizes = (C.c_long * 2)(5, 2 * chunk + 1)
    assert handle.bh_optim_workspace(sizes, 2) == 4 * 4 and handle.bh_optim_workspace((C.c_long * 1)(0), 1) == 0
    assert "n = 0" in _lib.last_error()

    def norm(g=ptrs, n=sizes, count=2, ctl=p, ws=p, ws_bytes=16, beta1=0.9, beta2=0.999, backoff=0.5):
        return handle.bh_optim_norm(g, n, count, ctl, 2.0, 1, 2.0, backoff, 2000, beta1, beta2, ws, ws_bytes, None), _lib.last_error()

    def update(p_=ptrs, g=ptrs, m=ptrs, v=ptrs, n=sizes, count=2, ctl=p, lr=2e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01):
        return handle.bh_optim_update(p_, g, m, v, n, count, ctl, lr, beta1, beta2, eps, wd, None), _lib.last_error()

    for kw, text in ((dict(g=None), "null pointer"), (dict(ctl=None), "null pointer"), (dict(ws=None), "null pointer"), (dict(n=None), "bad arguments"),
                     (dict(count=0), "n_tensors = 0"), (dict(n=(C.c_long * 2)(5, 0)), "n = 0"), (dict(n=(C.c_long * 2)(5, -3)), "n = -3"),
                     (dict(g=(C.c_void_p * 2)(4096, 0)), "gradient 1 is null"), (dict(g=(C.c_void_p * 2)(4098, 8192)), "gradient 0 is null or not 4-byte"),
                     (dict(beta1=1.0), "betas"), (dict(beta2=-0.1), "betas"), (dict(backoff=0.0), "loss scale rule"),
                     (dict(ws_bytes=12), "workspace of 12 bytes is too small"), (dict(ctl=C.c_void_p(4100)), "8-byte aligned")):
        rc, msg = norm(**kw)
        assert rc != 0 and text in msg, (kw, msg)
    for kw, text in ((dict(p_=None), "null pointer"), (dict(m=None), "null pointer"), (dict(ctl=None), "null pointer"), (dict(count=-1), "n_tensors = -1"),
                     (dict(n=(C.c_long * 2)(0, 5)), "n = 0"), (dict(v=(C.c_void_p * 2)(4096, 0)), "tensor 1 has a null"),
                     (dict(lr=-1e-3), "lr"), (dict(lr=float("inf")), "lr"), (dict(eps=-1.0), "eps"), (dict(wd=float("nan")), "weight_decay"),
                     (dict(beta1=1.5), "betas"), (dict(beta2=1.0), "betas")):
        rc, msg = update(**kw)
        assert rc != 0 and text in msg, (kw, msg)


# ---- checkpoints ------------------------------------------------------------------------------------------------------------------------
def test_a_state_dict_loads_into_torch_adamw_and_back(monkeypatch):
    """Host only: the device check is switched off and the state is filled by hand, no kernel runs."""
    monkeypatch.setattr(optim, "_devices", lambda named, what: None)
    torch.manual_seed(0)
    params = [torch.nn.Parameter(torch.randn(n)) for n in (4, 9)]
    ours = optim.AdamW(params, lr=1e-3, weight_decay=0.02, loss_scale=4096.0)
    for p in params:
        ours.state[p] = {"step": torch.tensor(0.0), "exp_avg": torch.randn_like(p), "exp_avg_sq": torch.rand_like(p)}
    ours.ctl[optim.CTL["step"]] = 7.0
    ours.ctl[optim.CTL["growth_tracker"]] = 5.0
    ours.param_groups[0]["lr"] = np.float64(1e-3)                    # what a LambdaLR over a numpy schedule leaves there
    saved = ours.state_dict()
    assert type(saved["param_groups"][0]["lr"]) is float
    blob = io.BytesIO()
    torch.save(saved, blob)
    blob.seek(0)
    assert torch.load(blob)["param_groups"] == saved["param_groups"]  # torch.load's default: weights only
    assert set(saved["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(saved["state"][1]["step"]) == 7.0
    assert saved["param_groups"][0]["loss_scale"] == 4096.0 and saved["param_groups"][0]["growth_tracker"] == 5

    theirs_params = [torch.nn.Parameter(p.detach().clone()) for p in params]
    theirs = torch.optim.AdamW(theirs_params, lr=5e-4, foreach=False)
    theirs.load_state_dict(copy.deepcopy(saved))                    # load_state_dict keeps the tensors it is given
    assert theirs.param_groups[0]["lr"] == 1e-3 and theirs.param_groups[0]["weight_decay"] == 0.02
    for p, q in zip(params, theirs_params):
        assert torch.equal(theirs.state[q]["exp_avg"], ours.state[p]["exp_avg"]) and float(theirs.state[q]["step"]) == 7.0
        q.grad = torch.ones_like(q)
    theirs.step()                                                     # torch takes the loaded state as its own: step 8
    back = theirs.state_dict()
    assert float(back["state"][0]["step"]) == 8.0 and theirs.param_groups[0]["decoupled_weight_decay"] is True
    assert back["param_groups"][0].pop("loss_scale") == 4096.0 and back["param_groups"][0].pop("growth_tracker") == 5      # torch carries them along

    again = optim.AdamW([torch.nn.Parameter(p.detach().clone()) for p in params], lr=2e-3, loss_scale=512.0)
    again.load_state_dict(back)                                       # a torch.optim.AdamW checkpoint: no loss scale in it, ours is kept
    c = again.control()
    assert c["step"] == 8.0 and c["beta1_pow"] == optim.beta_power(0.9, 8) and c["beta2_pow"] == optim.beta_power(0.999, 8) and c["scale"] == 512.0
    assert optim.beta_power(0.9, 3) == 0.9 * 0.9 * 0.9
    for q, r in zip(theirs_params, again.param_groups[0]["params"]):
        assert torch.equal(again.state[r]["exp_avg_sq"], theirs.state[q]["exp_avg_sq"])
    again.load_state_dict(saved)                                      # and ours: scale and tracker come back
    c = again.control()
    assert (c["step"], c["scale"], c["growth_tracker"]) == (7.0, 4096.0, 5.0)
    back["state"][1]["step"] = torch.tensor(3.0)
    with pytest.raises(ValueError, match="one step counter"):
        again.load_state_dict(back)

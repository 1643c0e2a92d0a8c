#!/usr/bin/env python3
"""
Record tests/golden/schedule_cases.json by EXECUTING THE REFERENCE on the CPU: bonito/schedule.py (the learning rate of every step of
the cases of tests/train_cases.py), bonito/training.py's ClipGrad (the max_norm it clips to before every step) and bonito/data.py's
load_numpy (which chunks land in the training and in the validation set). Run it only where the reference exists:

    python tests/golden/make_golden_schedule.py          # BONITO_REFERENCE names the checkout (default /root/reference)

bonito/schedule.py and bonito/data.py import numpy and torch only and are loaded by file path. bonito/training.py imports the whole
package; inert stub modules stand in for `bonito`, `bonito.util` and `tqdm`, none of which ClipGrad touches.
"""
import importlib.util
import json
import math
import os
import sys
import tempfile
import types

import numpy as np
import torch

REF = os.environ.get("BONITO_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import train_cases  # noqa: E402


def load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def ref_training(schedule):
    package = types.ModuleType("bonito")
    util = types.ModuleType("bonito.util")
    for name in ("accuracy", "decode_ref", "permute", "match_names", "tqdm_environ", "load_object"):
        setattr(util, name, None)
    package.schedule, package.util = schedule, util
    sys.modules.update({"bonito": package, "bonito.schedule": schedule, "bonito.util": util})
    if "tqdm" not in sys.modules:
        try:
            import tqdm  # noqa: F401
        except ImportError:
            stub = types.ModuleType("tqdm")
            stub.tqdm = None
            sys.modules["tqdm"] = stub
    return load_by_path("bonito.training", os.path.join(REF, "bonito", "training.py"))


def schedule_case(schedule, name, kwargs, lr, steps_per_epoch, epochs, last_epoch):
    param = torch.nn.Parameter(torch.zeros(1))
    optimizer = torch.optim.SGD([param], lr=lr)
    sched = getattr(schedule, name)(**kwargs)(optimizer, steps_per_epoch, epochs, last_epoch)
    lrs = []
    for _ in range((epochs - last_epoch) * steps_per_epoch):
        lrs.append(float(sched.get_last_lr()[0]))
        optimizer.step()
        sched.step()
    return lrs


def clip_case(training):
    clip = training.ClipGrad()
    param = torch.nn.Parameter(torch.zeros(4, dtype=torch.float64))
    max_norms = []
    for norm in train_cases.CLIP_NORMS:
        max_norms.append(float(clip.factor * np.quantile(clip.buffer, clip.quantile)))
        param.grad = torch.tensor([norm, 0.0, 0.0, 0.0], dtype=torch.float64)
        got = clip([param])
        assert (math.isnan(got) and math.isnan(norm)) or abs(got - norm) < 1e-12
    return max_norms


def data_case(data, name):
    with tempfile.TemporaryDirectory() as tmp:
        limit, valid_chunks = train_cases.write_data_case(tmp, name)
        train, valid = data.load_numpy(limit, tmp, valid_chunks=valid_chunks)
        out = {}
        for key, kwargs in (("train", train), ("valid", valid)):
            ds = kwargs["dataset"]
            out[key] = {"chunks_shape": list(ds.chunks.shape), "targets_shape": list(ds.targets.shape),
                        "ids": [int(v) for v in ds.lengths], "shuffle": bool(kwargs["shuffle"])}
        return out


def main():
    schedule = load_by_path("bonito.schedule", os.path.join(REF, "bonito", "schedule.py"))
    data = load_by_path("ref_bonito_data", os.path.join(REF, "bonito", "data.py"))
    training = ref_training(schedule)
    piece = schedule.piecewise_schedule([0.25, 0.5], [schedule.linear_schedule(0.0, 1.0), schedule.const_schedule(1.0),
                                                      schedule.cosine_decay_schedule(1.0, 0.1)])
    ts = [0.0, 0.1, 0.25, 0.3, 0.5, 0.75, 1.0]
    out = {
        "schedules": [schedule_case(schedule, *case) for case in train_cases.SCHEDULES],
        "clip_max_norms": clip_case(training),
        "piecewise": {"t": ts, "y": [float(piece(t)) for t in ts]},
        "inverse_sqrt": [float(schedule.inverse_sqrt_decay_schedule(3.0)(t)) for t in ts],
        "data": {name: data_case(data, name) for name in train_cases.DATA},
    }
    path = os.path.join(HERE, "schedule_cases.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()

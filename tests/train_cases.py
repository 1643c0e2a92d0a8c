"""The cases of tests/golden/schedule_cases.json, shared by the script that records them from the reference
(tests/golden/make_golden_schedule.py) and by tests/test_optim_ref_cpu.py, which replays them on bonito_amd."""
import os

import numpy as np

# (factory name, factory arguments, base lr, steps_per_epoch, epochs, last_epoch)
SCHEDULES = [
    ("linear_warmup_cosine_decay", {}, 2e-3, 4, 2, 0),                                     # the run of tests/test_gpu_train_cli.py
    ("linear_warmup_cosine_decay", {}, 2e-3, 4, 2, 1),
    ("linear_warmup_cosine_decay", {"end_ratio": 0.05, "warmup_steps": 5}, 1.0, 10, 3, 0),
    ("linear_warmup_cosine_decay", {"end_ratio": 0.05, "warmup_steps": 5}, 1.0, 10, 3, 1),
    ("linear_warmup_cosine_decay", {"warmup_steps": 0}, 5e-4, 7, 2, 0),
    ("linear_warmup_const_inverse_sqrt_decay", {"warmup_steps": 5, "decay_start_epoch": 2, "decay_scale": 1.0,
                                                "linear_cooldown_n_epochs": 1, "linear_cooldown_end_ratio": 0.1}, 1.0, 6, 6, 0),
    ("linear_warmup_const_inverse_sqrt_decay", {"warmup_steps": 5, "decay_start_epoch": 2, "decay_scale": 2.5,
                                                "linear_cooldown_n_epochs": 1, "linear_cooldown_end_ratio": 0.1}, 1.0, 6, 6, 2),
    ("linear_warmup_const_inverse_sqrt_decay", {"warmup_steps": 3, "decay_start_epoch": 1}, 3e-3, 5, 4, 0),
    ("linear_cooldown", {"end_ratio": 0.1}, 1.0, 5, 2, 0),
    ("linear_cooldown", {}, 2e-3, 5, 2, 1),
]

# gradient norms fed to ClipGrad one after the other (a NaN is not recorded); more than one turn of its buffer of 100
CLIP_NORMS = [float(v) for v in np.round(np.abs(np.random.default_rng(5).standard_normal(230)) * 3 + 0.2, 6)]
CLIP_NORMS[17] = float("nan")
CLIP_NORMS[140] = float("nan")

# name -> (chunks in the directory, chunks in validation/ or None, indices or None, limit, valid_chunks)
DATA = {
    "tail_3_percent": (100, None, None, 0, None),
    "tail_valid_chunks": (40, None, None, 32, 8),
    "tail_more_than_there_is": (10, None, None, 0, 25),
    "validation_directory": (32, 12, None, 32, 8),
    "validation_directory_no_limit": (32, 12, None, 0, None),
    "indices": (30, None, [29, 3, 31, 7, 0, 12, 40, 5], 0, 2),
    "indices_limit": (30, None, [29, 3, 31, 7, 0, 12, 40, 5], 4, 1),
}


def write_chunks(directory, n, first_id=0, indices=None, length=12):
    """n chunks whose reference_lengths are first_id, first_id + 1, ..: the lengths name the chunks a loader returned."""
    os.makedirs(directory, exist_ok=True)
    ids = np.arange(first_id, first_id + n)
    np.save(os.path.join(directory, "chunks.npy"), (ids[:, None] + np.arange(length)[None, :] / 100).astype(np.float32))
    np.save(os.path.join(directory, "references.npy"), np.tile(ids[:, None] % 4 + 1, (1, 6)).astype(np.uint8))
    np.save(os.path.join(directory, "reference_lengths.npy"), ids.astype(np.uint16))
    if indices is not None:
        np.save(os.path.join(directory, "indices.npy"), np.asarray(indices, dtype=np.int64))


def write_data_case(directory, name):
    """-> (limit, valid_chunks) of the case after writing its arrays under `directory`."""
    n, n_valid, indices, limit, valid_chunks = DATA[name]
    write_chunks(directory, n, indices=indices)
    if n_valid is not None:
        write_chunks(os.path.join(directory, "validation"), n_valid, first_id=1000)
    return limit, valid_chunks

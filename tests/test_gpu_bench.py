"""bench.py on a GPU box (-m gpu): the JSON contract of a short real run, and the N > 1 launch paths with real device work (the ranks share
the one GPU of the test box: more ranks than devices -> the barrier and the MAX-reduce go over gloo; on a multi-GPU node the same code takes
one rank per device over RCCL)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")


def _line(cmd, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-500:]          # stdout carries exactly one JSON line
    return json.loads(lines[0]), r.stderr


def test_single_rank_line_carries_roofline_and_the_contract_keys():
    j, _ = _line([sys.executable, "bench.py", "--model", "fast", "--steps", "24", "--warmup", "8", "--full", "--no-cpu-baseline",
                  "--no-side-legs"])
    for k in KEYS:
        assert k in j
    assert j["n_gpus"] == 1 and j["steps"] == 24 and j["scaling"] == "weak" and j["vs_baseline"] is None and j["data"] == "synthetic"
    assert j["value"] > 1e8 and abs(j["value"] - 512 * 10000 * 24 / (j["ms_per_step"] * 24e-3)) / j["value"] < 1e-6
    rf = j["roofline"]
    assert rf["bound"] == "mfma" and 0 < rf["frac"] < 1 and rf["unit"] == "TFLOP/s" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert "workload" in j["config"] and "model" not in j["config"]


def test_plain_run_times_the_headline_only_and_dumps_the_last_step(tmp_path):
    """Without --full the line carries the contract's keys and none of the side legs (the resident leg's regions only);
    --dump-outputs writes the decoder planes of the last timed step (the last --batch chunks of the last engine call, float32), two runs
    with the same arguments write the same arrays, and they are the outputs of that call's input batch - not of the call before it."""
    outs = []
    for i in range(2):
        d = tmp_path / str(i)
        j, _ = _line([sys.executable, "bench.py", "--steps", "8", "--warmup", "4", "--dump-outputs", str(d)])
        for k in KEYS:
            assert k in j
        assert j["steps"] == 8 and j["ms_per_step"] > 0 and abs(j["value"] - 512 * 10000 / (j["ms_per_step"] * 1e-3)) < 1e-3 * j["value"]
        assert len(j["regions_ms_per_step"]) == j["repeats"] >= 1 and j["with_h2d"] is None
        for k in ("with_h2d", "roofline", "kernel_ms_per_step", "per_call_1", "parity", "cpu_baseline", "e2e", "other_configs", "config1_ctc"):
            assert j[k] is None, k
        assert sorted(os.listdir(d)) == ["moves.npy", "qstring.npy", "sequence.npy"]
        got = {n: np.load(str(d / (n + ".npy"))) for n in ("sequence", "qstring", "moves")}
        shape = got["moves"].shape
        assert shape[0] == 512 and all(v.dtype == np.float32 and v.shape == shape for v in got.values())
        assert set(np.unique(got["moves"])) == {0.0, 1.0} and set(np.unique(got["sequence"])) <= {0.0, 65.0, 67.0, 71.0, 84.0}
        outs.append(got)
    for n, v in outs[0].items():
        assert np.array_equal(v, outs[1][n]), n
    # the same engine call outside the pipeline: model + decoder on the input batch of the last timed call, and of the call before it
    import torch
    import bench
    from bonito_amd import decode
    from bonito_amd.util import limit_host_threads
    a = bench.parse(["--steps", "8", "--warmup", "4"])
    calls = a.steps // a.per_call
    assert calls >= 2
    dev = torch.device("cuda", 0)
    # the seeded weights are bench.py's only under its host thread count: the recurrent layers' orthogonal init is a QR factorisation,
    # whose rounding depends on the number of threads
    threads = torch.get_num_threads()
    limit_host_threads(4)
    try:
        model = bench.build_model(a.model, a.call_batch, a.chunk)
        model.use_koi(batchsize=a.call_batch, chunksize=a.chunk, quantize=a.quantize)
        model = model.half().to(dev)
    finally:
        torch.set_num_threads(threads)
    signals = bench.input_batches(a, dev)
    dec = None

    def last_step(call):
        nonlocal dec
        with torch.no_grad():
            sc = model(signals[call % bench.N_BATCHES])
        if dec is None:
            dec = decode.CRFDecoder(a.call_batch, sc.shape[1], sc.shape[2], dev, mode=a.decoder)
        planes = dec.submit(sc).result()
        return {n: p[-a.batch:].numpy().astype(np.float32) for n, p in zip(("sequence", "qstring", "moves"), planes)}
    want, before = last_step(calls - 1), last_step(calls - 2)
    for n, v in outs[0].items():
        assert np.array_equal(v, want[n]), n
    assert not np.array_equal(outs[0]["sequence"], before["sequence"])


@pytest.mark.parametrize("launcher", ["self", "torchrun"])
def test_two_ranks_on_this_box_aggregate_over_the_slowest_rank(launcher):
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    tail = ["bench.py", "--gpus", "2", "--model", "fast", "--steps", "24", "--warmup", "8", "--full"]
    cmd = [sys.executable] + tail if launcher == "self" else [
        sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
        "--master-port", str(port)] + tail
    j, err = _line(cmd)
    assert j["n_gpus"] == 2 and j["steps"] == 24 and j["scaling"] == "weak"
    # whole-job aggregate: both ranks' samples over the slowest rank's time
    assert abs(j["value"] - 2 * 512 * 10000 * 24 / (j["ms_per_step"] * 24e-3)) / j["value"] < 1e-6
    assert abs(j["per_gpu"] * 2 - j["value"]) / j["value"] < 1e-9
    assert "rank 0/2" in err and "rank 1/2" in err                      # every rank says which device it drives
    assert j["cpu_baseline"] is None and j["other_configs"] is None      # rank 0, N = 1 only
    assert j["with_h2d"]["value"] > 0 and j["roofline"]["bound"] == "mfma"      # ... but the H2D leg and rank 0's roofline run at N > 1

"""The raw-to-chunk-rows path on the CPU, three ways: the reference itself (recorded in tests/golden/signal_cases.npz by
make_golden.py::make_signal_fixture), its line-by-line restatement (tests/signal_ref.py) and the product's host reader
(bonito_amd/reader.py + util.chunk + the fp16 cast). All three agree bit for bit on every case, so that tests/test_gpu_signal.py can
hold the device ingest to the restatement alone."""
import json
import os

import numpy as np
import pytest
import torch

import signal_ref
from bonito_amd import reader
from bonito_amd.signal import chunk_table
from bonito_amd.util import chunk

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "signal_cases.npz")


@pytest.fixture(scope="module")
def golden():
    return json.loads(str(np.load(GOLDEN)["meta"]))


@pytest.fixture(scope="module")
def restated(golden):
    out = []
    for g in golden:
        raw = signal_ref.make_raw(g["recipe"])
        out.append((raw, signal_ref.ingest(raw, g["scaling"], g["offset"], g["strategy"], g["params"], g["do_trim"])))
    return out


def test_fixture_holds_the_case_list(golden):
    """The fixture was generated from the case list the GPU sweep uses, and the recipes still give the same samples."""
    want = signal_ref.cases()
    assert [g["name"] for g in golden] == [c["name"] for c in want]
    for g, c in zip(golden, want):
        assert {k: g[k] for k in c} == json.loads(json.dumps(c)), g["name"]
        raw = signal_ref.make_raw(c["recipe"])
        assert (len(raw), signal_ref.digest(raw)) == (g["n"], g["raw_digest"]), g["name"]


def test_case_list_covers_what_it_is_meant_to(golden):
    """Checked against the reference's own results: the four weak combinations, both trim outcomes of every pair, every dtype."""
    quant = [g for g in golden if g["strategy"] is None or g["strategy"]["strategy"] == "quantile"]
    assert {(g["shift_python"], g["scale_python"]) for g in quant} == {(False, False), (True, False), (False, True), (True, True)}
    by = {g["name"]: g for g in golden}
    assert by["weak_shift"]["shift_python"] and not by["weak_shift"]["scale_python"]
    assert by["weak_scale"]["scale_python"] and not by["weak_scale"]["shift_python"]
    for name, flags in (("weak_shift_peak", (True, False)), ("weak_scale_peak", (False, True)), ("weak_both_peak", (True, True))):
        assert (by[name]["shift_python"], by[name]["scale_python"]) == flags and by[name]["trim"] == 210, name
    trims = {name: by[name]["trim"] for name in by if name.startswith("trim_")}
    assert trims == {"trim_no_peak": 10, "trim_peak_ends": 210, "trim_peak_to_limit": 10, "trim_peak_past_limit": 10,
                     "trim_peak_before_limit": 7970, "trim_past_max_trim": 10, "trim_below_max_trim": 290, "trim_at_max_trim": 330,
                     "trim_three_above": 10, "trim_four_above": 90, "trim_only_last_above": 10, "trim_last_above_rest_below": 290,
                     "trim_clipped_window_last_above": 10, "trim_clipped_window_last_below": 10, "trim_clipped_second_window": 10,
                     "trim_edge_raw2898": 10, "trim_edge_raw2899": 10, "trim_edge_raw2900": 90, "trim_off": 0}
    assert {g["signal_dtype"] for g in golden} == {"float32", "float64"}
    assert all(g["signal_dtype"] == "float32" for g in golden if g["shift_python"] and g["scale_python"])
    assert all(g["signal_dtype"] == "float64" for g in golden if not (g["shift_python"] and g["scale_python"]))


def test_restatement_equals_reference_fixture(golden, restated):
    for g, (raw, r) in zip(golden, restated):
        name = g["name"]
        assert (signal_ref.f64_bits(r["shift"]), signal_ref.f64_bits(r["scale"])) == (g["shift_bits"], g["scale_bits"]), name
        assert (signal_ref.is_python_scalar(r["shift"]), signal_ref.is_python_scalar(r["scale"])) == (g["shift_python"], g["scale_python"]), name
        assert r["trim"] == g["trim"], name
        assert (str(r["signal"].dtype), len(r["signal"])) == (g["signal_dtype"], g["signal_len"]), name
        assert signal_ref.digest(signal_ref.to_half(r["signal"])) == g["signal_digest"], name
        geoms = signal_ref.geometries_of(len(raw)) if len(r["signal"]) else []
        assert ["%d,%d" % lo for lo in geoms] == list(g["chunks"]), name
        for L, ov in geoms:
            rows = signal_ref.chunk_rows(r["signal"], L, ov)
            assert [rows.shape[0], signal_ref.digest(rows)] == g["chunks"]["%d,%d" % (L, ov)], (name, L, ov)


def test_reader_equals_restatement(golden, restated):
    """bonito_amd.reader.Read, then util.chunk and the cast, against the restatement: every scalar and every fp16 sample."""
    for g, (raw, r) in zip(golden, restated):
        name = g["name"]
        rd = reader.Read(name, raw, scaling=g["scaling"], offset=g["offset"], do_trim=g["do_trim"], scaling_strategy=g["strategy"],
                         norm_params=g["params"])
        assert (signal_ref.f64_bits(rd.shift), signal_ref.f64_bits(rd.scale)) == (g["shift_bits"], g["scale_bits"]), name
        assert (signal_ref.is_python_scalar(rd.shift), signal_ref.is_python_scalar(rd.scale)) == (g["shift_python"], g["scale_python"]), name
        assert rd.trimmed_samples == r["trim"], name
        assert rd.signal.dtype == np.float32 and len(rd.signal) == len(r["signal"]), name
        assert np.array_equal(torch.from_numpy(rd.signal).to(torch.float16).numpy().view(np.uint16),
                              signal_ref.to_half(r["signal"]).view(np.uint16)), name
        if len(rd.signal):
            for L, ov in signal_ref.geometries_of(len(raw)):
                got = chunk(torch.from_numpy(rd.signal), L, ov).to(torch.float16).numpy()
                want = signal_ref.chunk_rows(r["signal"], L, ov)
                assert got.shape == want.shape and np.array_equal(got.view(np.uint16), want.view(np.uint16)), (name, L, ov)


def test_trim_predicate_over_every_int16_value(golden, restated):
    """For the calibration, shift and scale of every case: which of the 65536 raw values count as above the trim threshold. The
    reference asks `scaled > scale * 2.4 + shift` on the pA signal; reader.py must ask exactly that (it used to ask `norm > 2.4` on the
    normalised signal, which rounds differently next to the threshold)."""
    every = np.arange(-32768, 32768).astype(np.int16)
    for g, (raw, r) in zip(golden, restated):
        scaled = float(g["scaling"]) * (every.astype(np.float32) + float(g["offset"]))
        want = signal_ref.above(scaled, r["threshold"])
        got = reader.above_threshold(scaled, r["shift"], r["scale"])
        assert want.dtype == got.dtype == np.bool_ and np.array_equal(want, got), (g["name"], int((want != got).sum()))


def test_chunk_table_addresses_the_rows_of_chunk(golden, restated):
    """signal.chunk_table (the origins the device kernel is launched with) against `chunk`: gathering the normalised signal at
    (start, available), tiled when short, gives the very rows, in order, for every case and chunk geometry."""
    for g, (raw, r) in zip(golden, restated):
        full = np.concatenate([np.zeros(r["trim"], r["signal"].dtype), r["signal"]])        # indexable by sample of the read
        for L, ov in signal_ref.geometries_of(len(raw)):
            reads, starts, avail = chunk_table([len(raw)], [r["trim"]], L, ov)
            assert (reads == 0).all() and (starts >= r["trim"]).all() and (starts + np.minimum(avail, L) <= len(raw)).all()
            rows = full[starts[:, None] + np.arange(L)[None, :] % avail[:, None]] if len(starts) else np.zeros((0, L))
            want = signal_ref.chunk(r["signal"], L, ov) if len(r["signal"]) else np.zeros((0, 1, L))
            assert rows.shape == want[:, 0].shape and np.array_equal(rows, want[:, 0]), (g["name"], L, ov)

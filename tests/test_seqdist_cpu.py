"""CTC-CRF sequence likelihood / forced alignment without a GPU: the fp64 restatement (tests/seqdist_ref.py) against the reference
fixture (tests/golden/crf_ctc_loss.npz, written by the reference's own ctc_loss / prepare_ctc_scores), against brute force, and
against the trusted CPU oracle for the free-start sum; the new ABI symbols; argument errors; the evaluate command's parser and data."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import seqdist_cases as sc_cases
import seqdist_ref as sr

ALPHABET = ["N", "A", "C", "G", "T"]


def fixture():
    return np.load(os.path.join(GOLDEN, "crf_ctc_loss.npz"))


def case_of(z, name):
    """-> dict with scores indexed [n, t, c] (float64 view of the fp16 values), layout flag, blank, targets, lengths, state_len"""
    sl = int(name[2])
    five = name.endswith("_5s")
    sc = z[name + "/scores"]
    return {"sl": sl, "five": five, "raw": sc, "scores": sc.transpose(1, 0, 2) if five else sc,
            "blank": None if five else float(z[name + "/blank"]), "targets": z[name + "/targets"], "lengths": z[name + "/lengths"]}


def dense_logz64(scores_ntc, sl, five, blank):
    """CTC_CRF.logZ (crf/model.py:47-52) in fp64 numpy, either layout."""
    S = 4 ** sl
    N, T = scores_ntc.shape[:2]
    j = np.arange(S)
    pred = np.stack([r * (S // 4) + j // 4 for r in range(4)], axis=1)
    alpha = np.zeros((N, S))
    for t in range(T):
        row = scores_ntc[:, t].astype(np.float64).reshape(N, S, 5 if five else 4)
        stay = row[:, :, 0] if five else blank
        mv = row[:, :, 1:] if five else row
        cand = np.concatenate([(alpha + stay)[:, :, None], alpha[:, pred] + mv], axis=2)
        alpha = np.logaddexp.reduce(cand, axis=2)
    return np.logaddexp.reduce(alpha, axis=1)


def test_fixture_holds_what_the_issue_asks_for():
    z = fixture()
    names = list(z["cases"])
    assert {n[:3] for n in names if n.endswith("_koi")} == {"sl1", "sl2", "sl3", "sl4", "sl5"}
    assert any(n.endswith("_5s") for n in names)
    for n in names:
        c = case_of(z, n)
        T = c["scores"].shape[1]
        assert c["lengths"].min() == c["sl"] and c["lengths"].max() > T
    five = case_of(z, "sl2_5s")["raw"].reshape(48, 4, 16, 5)[..., 0]
    assert np.unique(five).size > 8                                       # a non-constant stay column
    assert os.path.getsize(os.path.join(GOLDEN, "crf_ctc_loss.npz")) < 1 << 20


@pytest.mark.parametrize("name", ["sl1_koi", "sl2_koi", "sl3_koi", "sl4_koi", "sl5_koi", "sl1_5s", "sl2_5s", "sl3_5s"])
def test_restatement_matches_the_reference_fixture(name):
    z = fixture()
    c = case_of(z, name)
    lens = c["lengths"].astype(np.float64)
    seq = sr.log_scan(c["scores"], c["targets"], c["lengths"], c["sl"], c["five"], c["blank"])
    T = c["scores"].shape[1]
    feasible = c["lengths"] - c["sl"] <= T
    assert (np.isneginf(seq) == ~feasible).all()
    # normalise_scores=False: the reference's fp32 scan of the raw scores
    raw = -seq / lens
    ref = z[name + "/loss_raw_none"].astype(np.float64)
    assert np.isposinf(ref[~feasible]).all() and np.isposinf(raw[~feasible]).all()
    np.testing.assert_allclose(raw[feasible], ref[feasible], rtol=2e-5, atol=2e-5)
    # normalise_scores=True: the identity loss = -(seq_logz(raw) - logZ(raw)) / len against the reference's normalised scan
    lz = dense_logz64(c["scores"], c["sl"], c["five"], c["blank"])
    norm = -(seq - lz) / lens
    ref = z[name + "/loss_norm_none"].astype(np.float64)
    np.testing.assert_allclose(norm[feasible], ref[feasible], rtol=2e-5, atol=2e-5)
    assert np.isposinf(ref[~feasible]).all()
    assert np.isposinf(z[name + "/loss_norm_mean"]) and np.isposinf(z[name + "/loss_raw_mean"])
    clip = float(z["loss_clip"])
    np.testing.assert_allclose(np.clip(norm, 0.0, clip), z[name + "/loss_clip_none"], rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(np.clip(norm, 0.0, clip).mean(), z[name + "/loss_clip_mean"], rtol=2e-5)
    # Max scan: alignments are bit-comparable (scores on a grid of 1/8: every partial sum is exact), tie rule included
    align, best = sr.max_scan(c["scores"], c["targets"], c["lengths"], c["sl"], c["five"], c["blank"])
    assert (align == z[name + "/align"]).all()
    assert (align[~feasible] == -1).all() and np.isneginf(best[~feasible]).all()
    a = align[feasible]
    assert (a[:, -1] == (c["lengths"] - c["sl"])[feasible]).all() and (a[:, 0] <= 1).all() and (a >= 0).all()
    assert ((np.diff(a, axis=1) == 0) | (np.diff(a, axis=1) == 1)).all()
    ps = sr.path_score(c["scores"][feasible], c["targets"][feasible], c["lengths"][feasible], c["sl"], c["five"], a, c["blank"])
    assert (ps == best[feasible]).all()


@pytest.mark.parametrize("name", ["sl2_koi", "sl2_5s"])
def test_prepare_ctc_scores_equals_the_reference(name):
    from bonito_amd.crf.model import CTC_CRF
    from oracle import crf_ref
    z = fixture()
    c = case_of(z, name)
    x5 = c["raw"] if c["five"] else crf_ref.expand_blanks(c["raw"], np.float16(2.0)).transpose(1, 0, 2)
    stay, move = CTC_CRF(2, ALPHABET).prepare_ctc_scores(torch.from_numpy(np.ascontiguousarray(x5)),
                                                         torch.from_numpy(c["targets"].astype(np.int64)))
    assert stay.dtype == torch.float32
    assert (stay.numpy() == z[name + "/stay_scores"]).all() and (move.numpy() == z[name + "/move_scores"]).all()
    # ... and the restatement's index arithmetic gathers the same edges
    si, mi = sr.edge_indices(c["targets"], 2, True)
    x5n = np.ascontiguousarray(x5.transpose(1, 0, 2)).astype(np.float32)
    assert (np.take_along_axis(x5n, mi[:, None, :].repeat(x5n.shape[1], 1), 2).transpose(1, 0, 2) == z[name + "/move_scores"]).all()
    assert (np.take_along_axis(x5n, si[:, None, :].repeat(x5n.shape[1], 1), 2).transpose(1, 0, 2) == z[name + "/stay_scores"]).all()


@pytest.mark.parametrize("sl", [1, 2, 3])
@pytest.mark.parametrize("five", [False, True])
def test_scans_equal_exhaustive_enumeration(sl, five):
    rng = np.random.default_rng(100 + sl + 10 * five)
    C = (5 if five else 4) * 4 ** sl
    for T in (1, 3, 6, 8):
        for length in range(sl, sl + T + 2):
            sc = np.round(rng.normal(size=(1, T, C)) * 4) / 4            # a coarse grid: ties do occur
            tg = rng.integers(1, 5, size=(1, length)).astype(np.int8)
            lens = np.array([length], np.int32)
            tot, best, al = sr.enumerate_alignments(sc[0], tg[0], length, sl, five, 2.0)
            lz = sr.log_scan(sc, tg, lens, sl, five, 2.0)[0]
            a, b = sr.max_scan(sc, tg, lens, sl, five, 2.0)
            if al is None:
                assert np.isneginf(lz) and np.isneginf(b[0]) and (a == -1).all()
                continue
            assert abs(lz - tot) < 1e-9 and b[0] == best
            assert (a[0] == al).all(), (T, length, a[0], al)


@pytest.mark.parametrize("sl", [1, 2, 3])
def test_free_start_restatement_equals_the_oracle(sl):
    from oracle import crf_ref
    rng = np.random.default_rng(7 + sl)
    T, S = 24, 4 ** sl
    sc = (np.round(rng.normal(size=(T, 4 * S)) * 16) / 8).clip(-5, 5).astype(np.float16)
    for length in (0, 1, 2, 3, 4, 9, 20, 24, 25):
        seq = rng.integers(0, 4, size=length)
        text = "".join("ACGT"[b] for b in seq)
        lp, lz = crf_ref.seq_logprob(sc, sl, text, blank=2.0)
        mine = sr.free_start_logz(sc, seq, sl, 2.0)
        if length > T:
            assert np.isneginf(mine)
            continue
        assert abs(mine - lp) < 1e-9 * max(1.0, abs(lp)), (length, mine, lp)
        assert abs(dense_logz64(sc[None].astype(np.float64), sl, False, 2.0)[0] - lz) < 1e-9 * abs(lz)
    # a sequence of k bases or more: the free start dominates the fixed start (it sums over more paths)
    seq = rng.integers(0, 4, size=10)
    fixed = sr.log_scan(sc[None], (seq + 1)[None], np.array([10]), sl, False, 2.0)[0]
    assert sr.free_start_logz(sc, seq, sl, 2.0) > fixed


@pytest.mark.parametrize("sl", [4, 5])
def test_free_start_restatement_equals_the_oracle_at_long_state_lengths(sl):
    """State_len 4 and 5 on a short lattice, lengths on both sides of k: the sequence ends inside the dense levels, at the first chain
    position, and beyond; in both dtypes a sequence longer than T is -inf, not NaN."""
    from oracle import crf_ref
    rng = np.random.default_rng(70 + sl)
    T, S = 8, 4 ** sl
    sc = sc_cases.host_scores((T, 4 * S), 80 + sl)
    for length in list(range(sl + 3)) + [T, T + 1]:
        seq = rng.integers(0, 4, size=length)
        lp, _ = crf_ref.seq_logprob(sc, sl, "".join("ACGT"[b] for b in seq), blank=2.0)
        mine = sr.free_start_logz(sc, seq, sl, 2.0)
        if length > T:
            assert np.isneginf(lp) and np.isneginf(mine) and np.isneginf(sr.free_start_logz(sc, seq, sl, 2.0, dtype=np.float32))
            continue
        assert abs(mine - lp) < 1e-9 * max(1.0, abs(lp)), (length, mine, lp)
    assert abs(sr.free_start_logz(sc, [], sl, 2.0) - (T * 2.0 + sl * np.log(4.0))) < 1e-12       # the closed form of the empty sequence


def _free_short_rows(sl, T, scores, dtype):
    targets, lengths = sc_cases.free_short_case(sl, T)
    return np.array([sr.free_start_logz(scores, sc_cases.bases(targets, lengths, n), sl, sc_cases.BLANK, dtype=dtype)
                     for n in range(len(lengths))], np.float64)


@pytest.mark.parametrize("sl", sc_cases.FREE_STATE_LENS)
def test_free_start_fp32_run_agrees_with_fp64_on_the_short_cases(sl):
    """The fp32 run of the restatement is the yardstick of rows without a fixed-start chain: same finite / -inf pattern as fp64, and a
    distance of fp32 accumulation (measured 3.8e-9 .. 1.4e-5 over the 25 cases, the largest at state_len 5, T = 24, |logz| <= 65)."""
    for T in sc_cases.FREE_SHORT_T:
        scores = sc_cases.host_scores((T, 4 * 4 ** sl), 8000 + 100 * sl + T)
        _, lengths = sc_cases.free_short_case(sl, T)
        w64, w32 = _free_short_rows(sl, T, scores, np.float64), _free_short_rows(sl, T, scores, np.float32)
        assert not np.isnan(w64).any() and not np.isnan(w32).any()
        assert (np.isfinite(w64) == (lengths <= T)).all() and (np.isneginf(w64) == (lengths > T)).all()
        assert (np.isfinite(w32) == np.isfinite(w64)).all() and (np.isneginf(w32) == np.isneginf(w64)).all()
        fin = np.isfinite(w64)
        d = float(np.abs(w32[fin] - w64[fin]).max())
        print("sl %d T %d: fp32 run vs fp64 %.3e (|logz| <= %.1f)" % (sl, T, d, np.abs(w64[fin]).max()))
        # worst case of the roundings on the way to one result: per step two adds, the log-sum over four predecessors and the one with
        # the stay (six), then the running log-sum over the 4^k states; each within a spacing of the largest value
        assert d <= (6 * T + 4 ** sl) * np.spacing(np.float32(np.abs(w64[fin]).max()))
        assert abs(w64[0] - (T * sc_cases.BLANK + sl * np.log(4.0))) < 1e-12 and lengths[0] == 0


def _instance_from_workspace(handle, N, T, Lmax, k):
    """The instance row a launch selects, read from the host-only workspace query: its traceback words per step are waves x positions
    per thread, which differs from row to row."""
    words = (handle.bh_crf_seq_workspace(N, T, Lmax, k) - 512) // (N * T * 8)
    return [threads // 64 * per for threads, per in sc_cases.GEOMETRY].index(words)


def test_edge_cases_hold_every_row_class_and_reach_every_instance():
    """What tests/test_gpu_seqdist.py runs on the device, checked here without one: every class of row is in every free-start launch,
    the widened launch takes the 256 x 4 instance, and the instance sweeps select all seven rows of the list."""
    from bonito_amd import _lib
    handle = _lib.lib()
    assert len(sc_cases.GEOMETRY) == 7 and len({t // 64 * p for t, p in sc_cases.GEOMETRY}) == 7
    for sl in sc_cases.FREE_STATE_LENS:
        for T in sc_cases.FREE_SHORT_T:
            targets, lengths = sc_cases.free_short_case(sl, T)
            assert targets.dtype == (np.int32 if T % 2 else np.int8)
            have = set(lengths.tolist())
            assert have >= set(range(sl)) | {sl, T, T + 1}, (sl, T, have)           # 0, each of 1 .. k-1, k, just fits, cannot fit
            assert targets.shape[1] == lengths.max() == max(sl + 1, T + 1)
            assert ((targets != 0) == (np.arange(targets.shape[1])[None, :] < lengths[:, None])).all()
            assert lengths[-1] == min(sl + 1, T) and (targets[-1, :lengths[-1]] == targets[-1, 0]).all()
            row = _instance_from_workspace(handle, len(lengths), T, targets.shape[1], sl)
            assert row == sc_cases.chain_instance(targets.shape[1], sl) and sc_cases.GEOMETRY[row][0] == 64      # one wave
            wide = sc_cases.widen(targets)
            assert wide.shape[1] == sc_cases.WIDE and (wide[:, :targets.shape[1]] == targets).all() and not wide[:, targets.shape[1]:].any()
            row = _instance_from_workspace(handle, len(lengths), T, sc_cases.WIDE, sl)
            assert row == sc_cases.chain_instance(sc_cases.WIDE, sl) and sc_cases.GEOMETRY[row] == (256, 4)
            # ... so the four-wave launch mixes rows the prefix kernel finishes with rows the chain kernel finishes
            assert (lengths < sl).any() and (lengths >= sl).any()
    rows = set()
    for npos in sc_cases.NPOS:
        scores, targets, lengths = sc_cases.free_instance_case(npos)
        sl, (N, T) = sc_cases.FREE_INSTANCE_SL, scores.shape[:2]
        assert targets.shape == (3, npos + 1) and T == npos + 4 and lengths.tolist() == [npos + 1, npos + 1, max(2, npos - 1)]
        assert (targets[0] == targets[0, 0]).all() and (lengths >= sl).all() and (lengths <= T).all()          # every row finite
        assert ((targets != 0) == (np.arange(npos + 1)[None, :] < lengths[:, None])).all()
        row = _instance_from_workspace(handle, N, T, targets.shape[1], sl)
        assert row == sc_cases.chain_instance(targets.shape[1], sl)
        threads, per = sc_cases.GEOMETRY[row]
        assert npos <= threads * per and (row == 0 or npos > np.prod(sc_cases.GEOMETRY[row - 1]))
        rows.add(row)
        # the plain Log scan's sweep at state_len 1 (Lmax = npos) selects the same row
        assert _instance_from_workspace(handle, 2, npos + 67, npos, 1) == row
    assert rows == set(range(7))
    assert sc_cases.chain_instance(4097, 1) == -1 and handle.bh_crf_seq_workspace(2, 10, 4097, 1) == 0
    for T in sc_cases.TINY_T:
        for five in (False, True):
            raw, ntc, targets, lengths = sc_cases.tiny_log_case(T, five)
            k = sc_cases.TINY_SL
            assert lengths.tolist() == [k, k + 1, k + T, k + T + 1] and ntc.shape == (4, T, (5 if five else 4) * 4 ** k)
            want = sr.log_scan(ntc, targets, lengths, k, five, sc_cases.BLANK)
            assert np.isfinite(want[:3]).all() and np.isneginf(want[3])


def test_new_symbols_are_declared_bound_and_exported():
    from bonito_amd import _lib
    text = open(os.path.join(ROOT, "include", "bonito_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = _lib.lib()
    for name in ("bh_crf_seq_workspace", "bh_crf_seq_logz", "bh_crf_seq_viterbi", "bh_crf_seq_logz_free", "bh_crf_logz_dense"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and hasattr(handle, name)
    assert "bh_crf_posteriors" not in text                                # the opening comment named an undeclared function
    assert handle.bh_abi_version() == 1
    # the workspace query is host code: one traceback bit per cell, or the free start's per-step term, whichever is larger
    assert handle.bh_crf_seq_workspace(512, 1667, 250, 5) == 512 * 1667 * 4 * 8 + 512
    assert handle.bh_crf_seq_workspace(2, 10, 8, 3) == 2 * 10 * 8 + 512
    assert handle.bh_crf_seq_workspace(2, 10, 4100, 5) == 2 * 10 * 4096 // 8 + 512
    assert handle.bh_crf_seq_workspace(2, 10, 4101, 5) == 0                 # beyond the supported range: no silent truncation
    assert handle.bh_crf_seq_workspace(2, 10, 100, 6) == 0


def test_argument_errors_are_raised_without_a_device():
    from bonito_amd import _lib, decode
    from bonito_amd.crf.model import CTC_CRF
    from bonito_amd.nn import NoTorchCompute
    sd = CTC_CRF(3, ALPHABET)
    T, N, S = 12, 2, 64
    x5 = torch.zeros(T, N, 5 * S, dtype=torch.float16)
    x4 = torch.zeros(N, T, 4 * S, dtype=torch.float16)
    tg = torch.ones(N, 6, dtype=torch.int64)
    with pytest.raises(ValueError, match="shorter than state_len"):
        sd.ctc_loss(x5, tg, torch.tensor([6, 2]))
    with pytest.raises(ValueError, match="neither"):
        sd.ctc_loss(torch.zeros(T, N, 100, dtype=torch.float16), tg, torch.tensor([6, 6]))
    with pytest.raises(ValueError, match="blank_score"):
        sd.ctc_loss(x4, tg, torch.tensor([6, 6]))
    with pytest.raises(ValueError, match="lengths must lie"):
        sd.ctc_viterbi_alignments(x5, tg, torch.tensor([6, 7]))
    with pytest.raises(ValueError, match="labels"):
        sd.ctc_loss(x5, tg * 5, torch.tensor([6, 6]))
    with pytest.raises(ValueError, match="reduction"):
        sd.ctc_loss(x5, tg, torch.tensor([6, 6]), reduction="sum")
    with pytest.raises(NoTorchCompute):
        sd.ctc_loss(x5.float().requires_grad_(True), tg, torch.tensor([6, 6]))
    with pytest.raises(ValueError, match="free-start"):
        decode.seq_logz(x5, tg, torch.tensor([6, 6]), 3, free_start=True)
    with pytest.raises(_lib.HipEngineError):                                # valid arguments, host tensor: no CPU fallback
        sd.ctc_loss(x5, tg, torch.tensor([6, 6]))
    with pytest.raises(ValueError, match="outside ACGT"):
        decode.encode_sequences(["ACGN"])
    t, n = decode.encode_sequences(["ACGT", "", b"TT"])
    assert t.tolist() == [[1, 2, 3, 4], [0, 0, 0, 0], [4, 4, 0, 0]] and n.tolist() == [4, 0, 2]
    plane = torch.tensor([[0, 65, 0, 84], [0, 0, 0, 0]], dtype=torch.int8)
    t, n = decode.encode_sequences(plane)
    assert t.tolist() == [[1, 4], [0, 0]] and n.tolist() == [2, 0]
    assert hasattr(sd, "normalise")
    from bonito_amd.crf.model import SeqdistModel
    assert callable(SeqdistModel.loss) and callable(SeqdistModel.seq_logprob)


def test_evaluate_parser_and_data_loading(tmp_path):
    from bonito_amd.__main__ import modules
    from bonito_amd.cli import evaluate
    assert "evaluate" in modules
    args = evaluate.argparser().parse_args(["some/model", "--directory", str(tmp_path), "--chunks", "5", "--batchsize", "2",
                                            "--output_dir", str(tmp_path / "out"), "--standardise"])
    assert (args.dataset, args.chunks, args.batchsize, args.seed, args.device, args.weights) == ("valid", 5, 2, 9, "cuda", 0)
    assert args.standardise and args.output_dir == tmp_path / "out"
    assert "accuracy" in evaluate.argparser().description.lower()
    rng = np.random.default_rng(0)
    n = 20
    np.save(tmp_path / "chunks.npy", rng.normal(size=(n, 30)).astype(np.float32))
    refs = rng.integers(1, 5, size=(n, 9)).astype(np.uint8)
    lens = rng.integers(3, 10, size=n).astype(np.uint16)
    for i in range(n):
        refs[i, lens[i]:] = 0
    np.save(tmp_path / "references.npy", refs)
    np.save(tmp_path / "reference_lengths.npy", lens)
    ch, tg, ln = evaluate.load_chunks(tmp_path, "valid", 5)                  # no validation/: the tail split
    assert len(ln) == 5 and (tg == refs[-5:]).all() and (ln == lens[-5:]).all() and ch.shape == (5, 30)
    ch, tg, ln = evaluate.load_chunks(tmp_path, "train", 8)
    assert len(ln) == 0 or (tg == refs[:len(ln)]).all()
    os.mkdir(tmp_path / "validation")
    for f in ("chunks.npy", "references.npy", "reference_lengths.npy"):
        np.save(tmp_path / "validation" / f, np.load(tmp_path / f)[3:10])
    ch, tg, ln = evaluate.load_chunks(tmp_path, "valid", 4)
    assert (tg == refs[3:7]).all() and (ln == lens[3:7]).all()
    assert evaluate.decode_ref(np.array([1, 2, 0, 0]), ALPHABET) == "AC"

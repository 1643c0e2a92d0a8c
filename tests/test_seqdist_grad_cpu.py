"""Gradients of the CTC-CRF log-sums without a GPU: the alpha-beta restatement (tests/seqdist_grad_ref.py) against central differences
of the fp64 scans, against posteriors from exhaustive enumeration, the sum-to-one property the fixed-point combine of the kernel rests
on, the four new ABI symbols, and the argument errors of the new Python surface. The edge cases of tests/seqdist_cases.py that
tests/test_gpu_seqdist_grad.py runs on the device: they reach all seven instances at both edges and the four-wave row, hold every row
class, and the banded restatement those tests use is chain_grad bit for bit."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import seqdist_cases as sc_cases
import seqdist_ref as sr
import seqdist_grad_ref as gr

ALPHABET = ["N", "A", "C", "G", "T"]


def _case(sl, five, T=12, N=3, seed=0):
    rng = np.random.default_rng(1000 + 10 * sl + five + seed)
    C = (5 if five else 4) * 4 ** sl
    sc = rng.normal(0.0, 1.5, size=(N, T, C))
    Lmax = sl + T - 2
    lengths = np.array([sl, sl + T // 2, Lmax][:N], np.int32)
    targets = rng.integers(1, 5, size=(N, Lmax)).astype(np.int8)
    targets[1, :] = targets[1, 0]                                           # a homopolymer row: every position gathers the same elements
    targets[np.arange(Lmax)[None, :] >= lengths[:, None]] = 0
    return sc, targets, lengths


@pytest.mark.parametrize("five", [False, True])
@pytest.mark.parametrize("sl", [1, 2, 3])
def test_restatement_equals_central_differences(sl, five):
    """(a) h = 1e-5 in fp64: the truncation error of the difference quotient is ~ h^2 |f'''| / 6 ~ 1e-10 and its rounding error
    ~ eps |f| / h ~ 1e-9; measured largest difference 4.5e-10 (chain) - the bound 1e-7 is that of the finite difference, no kernel tolerance."""
    sc, targets, lengths = _case(sl, five)
    blank = None if five else 2.0
    N, T, C = sc.shape
    h = 1e-5
    chain = gr.chain_grad(sc, targets, lengths, sl, five, blank)
    _, dense = gr.dense_grad(sc, sl, five, blank)
    rng = np.random.default_rng(5)
    worst = [0.0, 0.0]
    si, mi = sr.edge_indices(targets, sl, five)
    for n in range(N):
        used = set(mi[n].tolist()) | (set(si[n].tolist()) if si is not None else set())
        cols = sorted(used)[:6] + rng.integers(0, C, size=3).tolist()
        for t in (0, T // 2, T - 1):
            for c in cols:
                up, dn = sc.copy(), sc.copy()
                up[n, t, c] += h
                dn[n, t, c] -= h
                fd = (sr.log_scan(up[n:n + 1], targets[n:n + 1], lengths[n:n + 1], sl, five, blank)[0]
                      - sr.log_scan(dn[n:n + 1], targets[n:n + 1], lengths[n:n + 1], sl, five, blank)[0]) / (2 * h)
                worst[0] = max(worst[0], abs(fd - chain["grad"][n, t, c]))
                fd = (sr.dense_logz(up[n:n + 1], sl, five, blank)[0] - sr.dense_logz(dn[n:n + 1], sl, five, blank)[0]) / (2 * h)
                worst[1] = max(worst[1], abs(fd - dense[n, t, c]))
    print("sl %d %s: restatement vs central differences: chain %.2e dense %.2e" % (sl, "5S" if five else "koi", *worst))
    assert worst[0] <= 1e-7 and worst[1] <= 1e-7


@pytest.mark.parametrize("five", [False, True])
@pytest.mark.parametrize("sl", [1, 2])
def test_restatement_equals_posteriors_from_enumeration(sl, five):
    """(b) every monotone alignment of one chunk, T <= 7: the posterior of an element = the probability mass of the alignments that use it."""
    import itertools
    rng = np.random.default_rng(40 + sl + 10 * five)
    C = (5 if five else 4) * 4 ** sl
    blank = None if five else 2.0
    for T in (1, 4, 7):
        for length in range(sl, sl + T + 2):
            sc = rng.normal(size=(1, T, C))
            tg = rng.integers(1, 5, size=(1, length)).astype(np.int8)
            if length % 2:
                tg[:] = tg[0, 0]
            got = gr.chain_grad(sc, tg, np.array([length]), sl, five, blank)
            n = length + 1 - sl
            if n - 1 > T:
                assert np.isneginf(got["logz"][0]) and not got["grad"].any()
                continue
            si, mi = sr.edge_indices(tg, sl, five)
            want = np.zeros((T, C))
            paths = []
            for steps in itertools.combinations(range(T), n - 1):
                pos, s, used = 0, 0.0, []
                for t in range(T):
                    if t in steps:
                        c = mi[0, pos]
                        pos += 1
                    else:
                        c = si[0, pos] if si is not None else None
                    s += sc[0, t, c] if c is not None else blank
                    used.append(c)
                paths.append((s, used))
            tot = np.logaddexp.reduce([s for s, _ in paths])
            for s, used in paths:
                for t, c in enumerate(used):
                    if c is not None:
                        want[t, c] += np.exp(s - tot)
            assert abs(got["logz"][0] - tot) < 1e-9
            assert np.abs(got["grad"][0] - want).max() < 1e-9, (T, length)


@pytest.mark.parametrize("five", [False, True])
@pytest.mark.parametrize("sl", [1, 2, 3])
def test_posteriors_of_a_step_sum_to_one(sl, five):
    """(c) a path takes exactly one edge per step: what lets the kernel combine a step's posteriors in 2^30 fixed point."""
    sc, targets, lengths = _case(sl, five, T=12, N=3, seed=3)
    blank = None if five else 2.0
    got = gr.chain_grad(sc, targets, lengths, sl, five, blank)
    assert np.isfinite(got["logz"]).all()
    assert np.abs(got["stay_total"] + got["move_total"] - 1.0).max() < 1e-9
    if five:
        assert np.abs(got["grad"].sum(axis=2) - 1.0).max() < 1e-9
    assert got["share"][1] >= lengths[1] - sl                                # the homopolymer row shares one element among all its edges
    _, dense = gr.dense_grad(sc, sl, five, blank)
    if five:
        assert np.abs(dense.sum(axis=2) - 1.0).max() < 1e-9
    else:
        assert (dense.sum(axis=2) <= 1.0 + 1e-9).all() and (dense >= 0).all()
    # a weight scales, an unreachable chunk gets zeros
    scaled = gr.chain_grad(sc, targets, lengths, sl, five, blank, weight=np.array([2.0, -1.0, 0.5]))
    assert np.abs(scaled["grad"] - got["grad"] * np.array([2.0, -1.0, 0.5])[:, None, None]).max() < 1e-12
    short = gr.chain_grad(sc[:, :3], targets, lengths, sl, five, blank)     # T = 3: only the one-position chunk still fits
    assert np.isfinite(short["logz"][0]) and np.isneginf(short["logz"][1:]).all() and not short["grad"][1:].any()


def test_gradient_symbols_are_declared_bound_and_exported():
    """(d) fails on the parent commit: the four entry points do not exist there."""
    from bonito_amd import _lib
    text = open(os.path.join(ROOT, "include", "bonito_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = _lib.lib()
    for name in ("bh_crf_seq_grad_workspace", "bh_crf_seq_logz_grad", "bh_crf_logz_dense_grad_workspace", "bh_crf_logz_dense_grad"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and hasattr(handle, name)
    assert handle.bh_abi_version() == 1
    # every alpha_t of the chain in fp32, positions rounded up to whole threads (the geometry table of the forward scan)
    assert handle.bh_crf_seq_grad_workspace(2, 10, 8, 3) == 2 * 10 * 6 * 4 + 512
    assert handle.bh_crf_seq_grad_workspace(2, 10, 70, 1) == 2 * 10 * 70 * 4 + 512
    assert handle.bh_crf_seq_grad_workspace(2, 10, 4100, 5) == 2 * 10 * 4096 * 4 + 512
    assert handle.bh_crf_seq_grad_workspace(2, 10, 4101, 5) == 0             # 4097 positions
    assert handle.bh_crf_seq_grad_workspace(2, 10, 100, 6) == 0
    assert handle.bh_crf_logz_dense_grad_workspace(3, 7, 2) == 3 * 7 * 16 * 4 + 512
    assert handle.bh_crf_logz_dense_grad_workspace(3, 7, 6) == 0 and handle.bh_crf_logz_dense_grad_workspace(0, 7, 2) == 0


def test_gradient_surface_refuses_host_tensors():
    """(e)"""
    from bonito_amd import _lib, decode
    from bonito_amd.crf.model import CTC_CRF
    from bonito_amd.nn import NoTorchCompute
    sd = CTC_CRF(3, ALPHABET)
    T, N, S = 12, 2, 64
    x5 = torch.zeros(T, N, 5 * S, dtype=torch.float16)
    x4 = torch.zeros(N, T, 4 * S, dtype=torch.float16)
    tg = torch.ones(N, 6, dtype=torch.int64)
    ln = torch.tensor([6, 6])
    with pytest.raises(_lib.HipEngineError):
        decode.seq_logz_grad(x5, tg, ln, 3)
    with pytest.raises(_lib.HipEngineError):
        decode.seq_logz_grad(x4, tg, ln, 3, blank_score=2.0)
    with pytest.raises(_lib.HipEngineError):
        decode.logz_grad(x5, 3)
    with pytest.raises(_lib.HipEngineError):
        sd.posteriors(x5)
    with pytest.raises(_lib.HipEngineError):
        sd.posteriors(x4, blank_score=2.0)
    with pytest.raises(ValueError, match="blank_score"):
        sd.posteriors(x4)
    with pytest.raises(ValueError, match="shorter than state_len"):
        decode.seq_logz_grad(x5, tg, torch.tensor([6, 2]), 3)
    with pytest.raises(ValueError, match="accumulate"):
        decode.seq_logz_grad(x5, tg, ln, 3, accumulate=True)
    for x in (x5.float().requires_grad_(True), x5.clone().requires_grad_(True)):
        with pytest.raises(NoTorchCompute):
            sd.ctc_loss(x, tg, ln)
        with pytest.raises(NoTorchCompute):                                  # ... before any other check
            sd.ctc_loss(x, tg, torch.tensor([6, 2]))
        with pytest.raises(NoTorchCompute):                                  # the plain scans return plain tensors
            decode.seq_logz(x, tg, ln, 3)
    assert "forward value only" not in (CTC_CRF.ctc_loss.__doc__ + decode.seq_logz.__doc__)


# ---- the cases tests/test_gpu_seqdist_grad.py runs on the device (tests/seqdist_cases.py), proved here without one -----------------------
def _grad_rows(handle, N, T, Lmax, k):
    """Positions kept per step by the gradient launch, from its host-only workspace query."""
    return (handle.bh_crf_seq_grad_workspace(N, T, Lmax, k) - 512) // (N * T * 4)


def test_gradient_cases_reach_every_instance_at_both_edges_and_the_four_wave_row():
    from bonito_amd import _lib
    handle = _lib.lib()
    k = sc_cases.GRAD_INSTANCE_SL
    edges, firsts = set(), []
    for npos in sc_cases.NPOS:
        for five in (False, True):
            raw, ntc, targets, lengths, wt = sc_cases.grad_instance_case(npos, five)
            Lmax, T = npos + 1, npos + 4
            assert raw.dtype == np.float16 and raw.shape == ((T, 5, 80) if five else (5, T, 64)) and ntc.shape[:2] == (5, T)
            assert targets.shape == (5, Lmax) and targets.dtype == np.int8
            assert lengths.tolist() == [Lmax, Lmax, max(2, Lmax - 2), k, min(k + 1, Lmax)] and (lengths - k <= T).all()
            assert wt.tolist() == [1.0, -1.0, 0.5, 0.0, 2.0]
            assert (targets[0] == targets[0, 0]).all() and (np.unique(targets[1]).size > 1 or npos < 64)
            assert ((targets != 0) == (np.arange(Lmax)[None, :] < lengths[:, None])).all()
            row = sc_cases.chain_instance(Lmax, k)
            threads, per = sc_cases.GEOMETRY[row]
            first = row == 0 and npos == 1 or row > 0 and npos == np.prod(sc_cases.GEOMETRY[row - 1]) + 1
            last = npos == threads * per
            assert first != last                                                # every size of NPOS is an edge of its row
            edges.add((row, "first" if first else "last"))
            if first and five:
                firsts.append(npos)
            # the library selects that row: the forward launch by its traceback words, the gradient by its alpha pitch
            words = (handle.bh_crf_seq_workspace(5, T, Lmax, k) - 512) // (5 * T * 8)
            assert [t // 64 * p for t, p in sc_cases.GEOMETRY].index(words) == row
            assert _grad_rows(handle, 5, T, Lmax, k) == -(-npos // per) * per
    assert edges == {(r, e) for r in range(7) for e in ("first", "last")}
    assert tuple(firsts) == sc_cases.GRAD_FIRST_SIZES                          # where the device test adds the flags
    for sl in sc_cases.GRAD_WIDE_SL:
        for T in sc_cases.GRAD_WIDE_T:
            for five in (False, True):
                raw, ntc, targets, lengths, wt = sc_cases.grad_wide_case(sl, T, five)
                S = 4 ** sl
                assert raw.shape == ((T, 5, 5 * S) if five else (5, T, 4 * S)) and targets.shape == (5, sc_cases.WIDE)
                assert lengths.tolist() == [sl, sl + 1, sl + (T + 1) // 2, sl + T, sl + T + 1]
                assert ((targets != 0) == (np.arange(sc_cases.WIDE)[None, :] < lengths[:, None])).all()
                assert (targets[3, :lengths[3]] == targets[3, 0]).all()
                row = sc_cases.chain_instance(sc_cases.WIDE, sl)
                assert row == 4 and sc_cases.GEOMETRY[row] == (256, 4)
                assert _grad_rows(handle, 5, T, sc_cases.WIDE, sl) == -(-(sc_cases.WIDE + 1 - sl) // 4) * 4
                # all but the first few of the 256 threads hold no position of any row
                assert (lengths.max() + 1 - sl + 3) // 4 <= 7


@pytest.mark.parametrize("five", [False, True], ids=["koi", "5S"])
def test_restatement_on_the_instance_cases(five):
    """Every row of grad_instance_case fits (finite logz); the homopolymer's share is its number of chain positions (5S: the stay
    edges of all of them gather one element; koi layout, where the stay edge has no element: its npos - 1 move edges do); in the 5S
    layout every step's posteriors sum to the row's weight."""
    k, blank = sc_cases.GRAD_INSTANCE_SL, None if five else sc_cases.BLANK
    for npos in sc_cases.NPOS:
        raw, ntc, targets, lengths, wt = sc_cases.grad_instance_case(npos, five)
        r = gr.chain_grad_banded(ntc, targets, lengths, k, five, blank, weight=wt)
        assert np.isfinite(r["logz"]).all(), npos
        assert r["share"][0] == (npos if five else npos - 1)
        assert np.abs(r["stay_total"] + r["move_total"] - 1.0).max() < 1e-9
        if five:
            assert np.abs(r["grad"].sum(axis=2) - wt[:, None]).max() < 1e-9
        assert not r["grad"][3].any()


@pytest.mark.parametrize("five", [False, True], ids=["koi", "5S"])
@pytest.mark.parametrize("sl", sc_cases.GRAD_WIDE_SL)
def test_restatement_on_the_widened_cases(sl, five):
    """-inf for exactly the row meant not to fit, finite for the others; the homopolymer (a move at every step) shares one element
    among its T + 1 stay edges (koi layout: its T move edges); 5S: a step's posteriors sum to the weight, to zero where nothing fits."""
    blank = None if five else sc_cases.BLANK
    for T in sc_cases.GRAD_WIDE_T:
        raw, ntc, targets, lengths, wt = sc_cases.grad_wide_case(sl, T, five)
        r = gr.chain_grad(ntc, targets, lengths, sl, five, blank, weight=wt)
        assert np.isfinite(r["logz"][:4]).all() and np.isneginf(r["logz"][4])
        assert r["share"][3] == (T + 1 if five else T)
        assert not r["grad"][4].any()
        if five:
            assert np.abs(r["grad"].sum(axis=2) - np.where(np.arange(5) < 4, wt, 0.0)[:, None]).max() < 1e-9
        for dtype in (np.float64, np.float32):
            a = gr.chain_grad(ntc, targets, lengths, sl, five, blank, weight=wt, dtype=dtype)
            b = gr.chain_grad_banded(ntc, targets, lengths, sl, five, blank, weight=wt, dtype=dtype)
            assert all(np.array_equal(a[key], b[key]) for key in ("logz", "grad", "share"))


@pytest.mark.parametrize("five", [False, True], ids=["koi", "5S"])
def test_banded_restatement_is_chain_grad_bit_for_bit(five):
    """chain_grad_banded skips only cells where chain_grad adds an exact zero: logz, grad and share equal chain_grad's bit for bit, in
    fp64 and in fp32, on the instance cases up to 257 positions (rows of Lmax, Lmax - 2, k and k + 1 labels, weights of both signs and
    zero) - and on every widened case, a row that cannot fit included (the test above)."""
    k, blank = sc_cases.GRAD_INSTANCE_SL, None if five else sc_cases.BLANK
    for npos in [n for n in sc_cases.NPOS if n <= 257]:
        raw, ntc, targets, lengths, wt = sc_cases.grad_instance_case(npos, five)
        for dtype in (np.float64, np.float32):
            a = gr.chain_grad(ntc, targets, lengths, k, five, blank, weight=wt, dtype=dtype)
            b = gr.chain_grad_banded(ntc, targets, lengths, k, five, blank, weight=wt, dtype=dtype)
            assert all(np.array_equal(a[key], b[key]) for key in ("logz", "grad", "share")), (npos, dtype)
            assert a["grad"].dtype == b["grad"].dtype == dtype
            assert np.abs(a["stay_total"] - b["stay_total"]).max() < 1e-6 and np.abs(a["move_total"] - b["move_total"]).max() < 1e-6

"""Gradients of the CTC-CRF log-sums without a GPU: the alpha-beta restatement (tests/seqdist_grad_ref.py) against central differences
of the fp64 scans, against posteriors from exhaustive enumeration, the sum-to-one property the fixed-point combine of the kernel rests
on, the four new ABI symbols, and the argument errors of the new Python surface."""
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
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

"""Without a GPU: the fp64 restatements and tolerances of tests/ctc_kernels_ref.py reject a subtly wrong kernel on the very inputs the GPU
suite (tests/test_gpu_ctc_kernels.py) uses, the run semantics of the greedy oracle, the new ABI entry point, and every host-side refusal
of the four launchers (dummy pointers: each case is refused in front of any device call)."""
import ctypes as C

import numpy as np
import pytest

import ctc_kernels_ref as kr
from oracle import ctc_ref


def _rejects(got, ref, tol):
    return not kr.within(np.asarray(got).astype(np.float16), ref, tol)[0]


HEAD_CASES = [(c, F) for c in kr.HEAD_CLASSES[1:] for F in kr.HEAD_FEATURES]


@pytest.mark.parametrize("classes,F", HEAD_CASES)
def test_head_reference_rejects_planted_errors(classes, F):
    for M in kr.HEAD_ROWS:
        for large in ((False, True) if M == kr.HEAD_ROWS[-1] else (False,)):         # the large-logit case runs at the largest M alone
            x, w, b = kr.head_inputs(classes, F, M, large)
            ref, tol = kr.ctc_head(x, w, b)
            x64, w64, b64 = x.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
            logits = x64 @ w64.T + b64
            assert kr.within(ref.astype(np.float16), ref, tol)[0]                   # the rounded truth passes
            assert abs(np.exp(ref).sum(axis=-1) - 1).max() < 1e-12
            # the last 8 features dropped
            assert _rejects(kr.log_softmax64(x64[:, :F - 8] @ w64[:, :F - 8].T + b64), ref, tol), (M, large)
            # no bias
            assert _rejects(kr.log_softmax64(logits - b64), ref, tol), (M, large)
            # two classes swapped
            assert _rejects(ref[:, ::-1] if classes == 2 else ref[:, [1, 0] + list(range(2, classes))], ref, tol), (M, large)
            # the softmax over 8 classes: the padding as logits of 0 instead of -inf
            if classes < 8:
                padded = np.concatenate([logits, np.zeros((M, 8 - classes))], axis=1)
                assert _rejects(kr.log_softmax64(padded)[:, :classes], ref, tol), (M, large)


def test_head_of_one_class_is_exactly_zero_and_large_logits_need_the_shift():
    x, w, b = kr.head_inputs(1, 256, 257)
    ref, tol = kr.ctc_head(x, w, b)
    assert not ref.any()
    x, w, b = kr.head_inputs(5, 16, 600, large=True)
    logits = x.astype(np.float64) @ w.astype(np.float64).T + b
    assert logits.max() > 60 and logits.min() < -60
    ref, tol = kr.ctc_head(x, w, b)
    assert np.isfinite(ref).all() and kr.head_row_sum_tolerance(ref, tol).max() < 1e-2


NORM_CASES = [(D, M) for D in kr.NORM_D for M in kr.NORM_M]


@pytest.mark.parametrize("D,M", NORM_CASES)
def test_rmsnorm_reference_rejects_planted_errors(D, M):
    a, x, w = kr.norm_inputs(D, M)
    a64, x64, w64 = a.astype(np.float64), x.astype(np.float64), w.astype(np.float64)
    caught = dict(eps=False, alpha=False)
    for eps in kr.NORM_EPS:
        for alpha in kr.NORM_ALPHA:
            for xin in (x, None):
                ref, tol = kr.rmsnorm_residual(a, xin, w, alpha, eps)
                assert kr.within(ref.astype(np.float16), ref, tol)[0]
                al = float(np.float32(alpha))
                z = a64 + al * x64 if xin is not None else a64
                ms = (z * z).mean(axis=-1, keepdims=True)
                # eps outside the root: shows on the rows whose mean square is of eps's size (from M = 3 on)
                caught["eps"] |= _rejects(z / (np.sqrt(ms) + eps) * w64, ref, tol)
                # alpha ignored
                if xin is not None and alpha != 1.0:
                    caught["alpha"] = True
                    z1 = a64 + x64
                    assert _rejects(z1 / np.sqrt((z1 * z1).mean(axis=-1, keepdims=True) + eps) * w64, ref, tol), (alpha, eps)
                # the second vector of a lane dropped: statistics over the first 512 elements, nothing stored behind them
                if D > 512:
                    ms1 = (z[:, :512] ** 2).sum(axis=-1, keepdims=True) / D
                    wrong = z / np.sqrt(ms1 + eps) * w64
                    wrong[:, 512:] = 0.0
                    assert _rejects(wrong, ref, tol), (alpha, eps)
                    assert _rejects(z / np.sqrt(ms1 + eps) * w64, ref, tol), (alpha, eps)
                # the mean over nv * 8 rounded up to 512
                if D % 512:
                    ms2 = (z * z).sum(axis=-1, keepdims=True) / (-(-D // 512) * 512)
                    assert _rejects(z / np.sqrt(ms2 + eps) * w64, ref, tol), (alpha, eps)
                if M >= 3:
                    assert not ref[0].any() and np.isfinite(ref).all()
                    assert (z[1] ** 2).sum() > 65504.0 and (z[1] ** 2).sum() < 3e38
    assert caught["alpha"] and (caught["eps"] or M < 3)


def test_greedy_oracle_run_semantics():
    alphabet = "NACGT"
    p = np.full((3, 5), 0.05)
    # a run that ends at the end of the read: its quality is the mean over both steps, its path its first step
    p[0, 0], p[1, 1], p[2, 1] = 0.8, 0.8, 0.6
    p /= p.sum(axis=1, keepdims=True)
    seq, qs, path, qf = ctc_ref.viterbi_search(np.log(p).astype(np.float32), alphabet, 1.0, 0.0, return_qfloat=True)
    assert (seq, path) == ("A", [1])
    want = -10 * np.log10(1 - (p[1, 1] + p[2, 1]) / 2)
    assert abs(qf[0] - want) < 1e-5 and qs == chr(33 + int(round(want)))
    # runs of one step: the same label again after a blank is a new base
    p = np.full((3, 5), 0.05)
    p[0, 2], p[1, 0], p[2, 2] = 0.8, 0.8, 0.7
    p /= p.sum(axis=1, keepdims=True)
    seq, qs, path, qf = ctc_ref.viterbi_search(np.log(p).astype(np.float32), alphabet, 2.0, 1.0, return_qfloat=True)
    assert (seq, path) == ("CC", [0, 2])
    assert np.abs(qf - (-20 * np.log10(1 - p[[0, 2], 2]) + 1)).max() < 1e-5
    # the same label on adjacent steps is ONE base; p = 1 clamps the error to 1e-4; an empty read
    lp = np.full((2, 5), -np.inf, np.float32)
    lp[:, 3] = 0.0
    assert ctc_ref.viterbi_search(lp, alphabet, 1.0, 0.0) == ("G", chr(33 + 40), [0])
    assert ctc_ref.viterbi_search(np.zeros((0, 5), np.float32), alphabet) == ("", "", [])
    # the plain call returns what it returned before the option existed
    assert ctc_ref.viterbi_search(np.log(p).astype(np.float32), alphabet, 2.0, 1.0) == (seq, qs, path)


def test_greedy_inputs_hold_the_planted_cases():
    for Cn in kr.GREEDY_CLASSES:
        reads = kr.greedy_reads(Cn)
        assert sorted(set(len(r) for r in reads)) == sorted(kr.GREEDY_LENGTHS)
        a = reads[0].argmax(axis=1)
        assert a[-1] == a[-2] == 1 and a[-3] == 0 and reads[1].argmax(axis=1)[:2].tolist() == [1, 0]
        assert (reads[2].argmax(axis=1) == Cn - 1).all() and not reads[3].argmax(axis=1).any()
        srt = np.sort(reads[4], axis=1)
        assert (srt[:, -1] == srt[:, -2]).sum() > 20 and (srt[:, 0] == srt[:, -1]).sum() >= 15
        assert np.isneginf(reads[5]).any() and (reads[5].max(axis=1) == 0).sum() > 50
        # runs longer than a thread's segment, ceil(T / 256) steps
        lab = reads[9].argmax(axis=1)
        edges = np.flatnonzero(np.diff(lab)) + 1
        assert len(lab) == 1300 and np.diff(np.concatenate([[0], edges, [1300]])).max() > 6


def test_q_tolerance_is_small_and_grows_only_towards_the_clamp():
    for qscale, qbias in kr.GREEDY_QPARAMS:
        e = np.array([1.0, 0.5, 1e-2, 1e-4])
        tol = kr.greedy_q_tolerance(-10 * np.log10(e) * qscale + qbias, qscale, qbias)
        assert (np.diff(tol) > 0).all() and tol[0] < 1e-5 and tol[2] < 5e-4 and tol[3] < 0.04


def test_beam_lanes_restates_the_launcher():
    assert [kr.beam_lanes(c, b) for c, b in kr.BEAM_PAIRS] == [64, 32, 16, 16, 64, 64]


def test_worst_fill_reads_fill_the_candidate_arrays_and_the_node_pool():
    """The reads of the GPU suite's worst-fill case (8 classes, beam 16, threshold 0, T = 50): the near-flat ones reach B * C = 128
    candidates in a step; the forking ones allocate B new nodes in every step once the beam is full (1, 2, 4, 8 survivors in the first
    four steps), which is the pool's bound of 1 + T * B less what those first steps cannot use."""
    Cn, B, T = 8, 16, 50
    fill = [kr.beam_fill(lp, B, 0.0) for lp in kr.beam_reads(Cn, kr.beam_lanes(Cn, B) + 1, flat=True, T=T)]
    assert max(most for most, _ in fill[1:]) == B * Cn and all(most <= B * Cn and nodes <= 1 + T * B for most, nodes in fill)
    for most, nodes in fill[::4]:
        assert most == B * Cn and nodes >= 1 + 2 + 4 + 8 + 16 + B * (T - 4)


def test_ctc_head_symbol_is_declared_bound_and_exported():
    import os
    import re
    from conftest import ROOT
    from bonito_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bonito_hip.h")).read(), flags=re.S)
    assert re.search(r"\bbh_ctc_head\s*\(", code) and "bh_ctc_head" in _lib.SIGNATURES and hasattr(_lib.lib(), "bh_ctc_head")


P = C.c_void_p(4096)


def _head(classes=5, F=64, M=10, **ptr):
    from bonito_amd import _lib
    a = dict(x=P, w=P, b=P, out=P)
    a.update(ptr)
    return _lib.lib().bh_ctc_head(a["x"], a["w"], a["b"], a["out"], M, F, classes, None), _lib.last_error()


def _norm(D=64, M=10, **ptr):
    from bonito_amd import _lib
    a = dict(a=P, x=P, w=P, out=P)
    a.update(ptr)
    return _lib.lib().bh_rmsnorm_residual(a["a"], a["x"], a["w"], a["out"], M, D, 1.0, 1e-5, None), _lib.last_error()


def _greedy(classes=5, R=3):
    from bonito_amd import _lib
    return _lib.lib().bh_ctc_greedy_decode(P, P, R, classes, 1.0, 0.0, P, P, P, P, None), _lib.last_error()


def _beam(classes=5, R=3, beam=5, thr=1e-3):
    from bonito_amd import _lib
    return _lib.lib().bh_ctc_beam_search(P, P, R, classes, beam, thr, P, P, P, P, None), _lib.last_error()


def test_head_refusals_on_the_host():
    for kw in (dict(classes=0), dict(classes=9), dict(F=0), dict(F=12)):
        rc, msg = _head(**kw)
        assert rc != 0 and msg.startswith("ctc_head:") and "classes<=8 and features%8==0" in msg, (kw, msg)
    rc, msg = _head(classes=8, F=2056)                          # 8 * 2056 * 4 bytes = 64 KiB + 256
    assert rc != 0 and "do not fit 64 KiB of LDS" in msg and "8 classes x 2056 features" in msg, msg
    rc, msg = _head(classes=5, F=3280)                          # 65600 bytes
    assert rc != 0 and "do not fit 64 KiB of LDS" in msg, msg
    for kw in (dict(x=None), dict(w=None), dict(b=None), dict(out=None), dict(M=0)):
        rc, msg = _head(**kw)
        assert rc != 0 and "ctc_head: bad arguments" in msg, (kw, msg)


def test_rmsnorm_refusals_on_the_host():
    for D in (0, 4, 1032):
        for x in (P, None):                                     # with the residual and without
            rc, msg = _norm(D=D, x=x)
            assert rc != 0 and "D must be a multiple of 8 and <= 1024 (got %d)" % D in msg, (D, msg)
    for kw in (dict(a=None), dict(w=None), dict(out=None), dict(M=0)):
        rc, msg = _norm(**kw)
        assert rc != 0 and "rmsnorm_residual: bad arguments" in msg, (kw, msg)


def test_decoder_refusals_on_the_host():
    for kw in (dict(classes=1), dict(classes=9), dict(R=0)):
        rc, msg = _greedy(**kw)
        assert rc != 0 and msg.startswith("ctc_greedy:") and "2 <= classes <= 8" in msg, (kw, msg)
        rc, msg = _beam(**kw)
        assert rc != 0 and msg.startswith("ctc_beam:") and "2 <= classes <= 8" in msg, (kw, msg)
    for beam in (0, 17):
        rc, msg = _beam(beam=beam)
        assert rc != 0 and "beam_size must be in 1..16 (got %d)" % beam in msg, msg
    for thr in (-0.1, 1.0):
        rc, msg = _beam(thr=thr)
        assert rc != 0 and "threshold must be in [0, 1)" in msg, (thr, msg)


def test_all_empty_batches_decode_to_empty_results_without_a_device():
    """No launch and no device allocation: a batch whose reads are all empty has nothing to hand to a kernel."""
    import torch
    from bonito_amd.ctc import decode
    empty = [torch.zeros(0, 5), torch.zeros(0, 5)]
    assert decode.viterbi_search_batch(empty, "NACGT") == [("", "", []), ("", "", [])]
    assert decode.beam_search_batch(empty, "NACGT") == [("", []), ("", [])]
    assert decode.viterbi_search_batch([], "NACGT") == [] and decode.beam_search_batch([], "NACGT") == []

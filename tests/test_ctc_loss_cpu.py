"""The CTC loss of bonito.ctc without a GPU: the fp64 restatement (tests/ctc_loss_ref.py) against the enumeration of every alignment,
against the fixture recorded from the reference's own Model.ctc_label_smoothing_loss and torch's fp64 ctc_loss
(tests/golden/ctc_loss.npz), the sum-to-one property the kernel's fixed-point combine rests on, the new ABI symbols, and every argument
error of the C entry points and of the Python surface (all found on the host, before anything is launched)."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import ctc_loss_ref as cr

CASES = ["t40_c2", "t48_c5", "t48_inf"]


def _case(name):
    z = np.load(os.path.join(GOLDEN, "ctc_loss.npz"))
    c = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}
    x = c["logits"].astype(np.float64)
    c["lp64"] = x - np.logaddexp.reduce(x, axis=-1, keepdims=True)
    c["lp32"] = torch.log_softmax(torch.from_numpy(c["logits"]), dim=-1).numpy()          # what the reference was given
    return c


def _collapse(path):
    out, last = [], 0
    for c in path:
        if c != last and c != 0:
            out.append(c)
        last = c
    return out


def test_restatement_equals_enumeration_of_every_alignment():
    """Every path in C^T whose collapse (merge repeats, drop blanks) is the target, T <= 6, C = 3: nll and the class occupancy of
    every step. fp64 against fp64: the bound 1e-12 is summation rounding of at most 729 terms."""
    rng = np.random.default_rng(7)
    Cn = 3
    for T in (1, 2, 3, 5, 6):
        lp = rng.normal(size=(T, Cn)) * 1.5
        lp -= np.logaddexp.reduce(lp, axis=-1, keepdims=True)
        for target in ([], [1], [2, 2], [1, 2], [1, 1, 2], [2, 1, 2], [1, 1, 1], [1, 2, 1, 2]):
            tot, occ = 0.0, np.zeros((T, Cn))
            for path in itertools.product(range(Cn), repeat=T):
                if _collapse(path) == target:
                    pr = np.exp(sum(lp[t, c] for t, c in enumerate(path)))
                    tot += pr
                    for t, c in enumerate(path):
                        occ[t, c] += pr
            nll, got, _ = cr.ctc_chunk(lp, target)
            if tot == 0.0:
                assert np.isposinf(nll) and not got.any(), (T, target)
                continue
            assert abs(nll + np.log(tot)) < 1e-12, (T, target)
            assert np.abs(got - occ / tot).max() < 1e-12, (T, target)


@pytest.mark.parametrize("name", CASES)
def test_restatement_equals_the_recorded_reference(name):
    """The loss dict against the reference's own fp32 run (on fp32 and on fp16 log_probs): the reference sums T terms per chunk in
    fp32, so the two may differ by T roundings, 2^-23 T relative. Per-chunk nll and the gradient with respect to the logits (after
    log_softmax's backward  g - exp(lp) sum_c g  with g = -occ) against torch's fp64 run: fp64 against fp64, 1e-9."""
    c = _case(name)
    T, N, Cn = c["logits"].shape
    fin = np.isfinite(c["nll64"])
    if name == "t48_inf":
        assert fin.sum() == 1 and (~fin).sum() == 3
    for tag, lp in (("ref32", c["lp32"]), ("ref16", c["lp32"].astype(np.float16))):
        d = cr.loss_dict(lp.astype(np.float64), c["targets"], c["lengths"])
        want = c[tag]
        for got, ref in zip((d["total_loss"], d["loss"], d["label_smooth_loss"]), want):
            print("%s %s: restatement %.9g reference %.9g" % (name, tag, got, ref))
            if np.isinf(ref):
                assert np.isposinf(got)
            else:
                assert abs(got - ref) <= 2.0 ** -23 * T * abs(ref)
    r = cr.ctc_loss_ref(c["lp64"], c["targets"], c["lengths"])
    assert np.isposinf(r["nll"][~fin]).all() and not r["occ"][:, ~fin].any()
    assert np.abs(r["nll"][fin] - c["nll64"][fin]).max() <= 1e-9
    proj = cr.logsoftmax_projection(-r["occ"], c["lp64"])
    assert np.abs(proj - c["grad_logits64"]).max() <= 1e-9
    if "total_grad_logits64" in c:
        w = cr.default_weights(Cn)
        g = -r["occ"] / np.maximum(c["lengths"], 1)[None, :, None] / N - w[None, None, :] / (T * N * Cn)
        assert np.abs(cr.logsoftmax_projection(g, c["lp64"]) - c["total_grad_logits64"]).max() <= 1e-9
        assert abs(cr.loss_dict(c["lp64"], c["targets"], c["lengths"])["total_loss"] - c["total64"]) <= 1e-9


@pytest.mark.parametrize("name", CASES)
def test_occupancy_of_every_step_sums_to_one(name):
    """A path is in exactly one state per step: what lets the kernel combine a step's occupancies in 2^30 fixed point."""
    c = _case(name)
    r = cr.ctc_loss_ref(c["lp64"], c["targets"], c["lengths"])
    fin = np.isfinite(r["nll"])
    assert fin.any()
    assert np.abs(r["occ"][:, fin].sum(axis=-1) - 1.0).max() < 1e-9
    assert (r["occ"] >= 0).all()


def test_definitions_where_torch_gives_nan():
    rng = np.random.default_rng(3)
    lp = rng.normal(size=(12, 2, 5))
    lp -= np.logaddexp.reduce(lp, axis=-1, keepdims=True)
    lp[:, :, 4] = -np.inf                                                   # class 4 can never be emitted
    tg = np.array([[1, 2, 3, 1], [1, 4, 2, 0]])
    r = cr.ctc_loss_ref(lp, tg, [4, 3], weights=[0.4, 0.2, 0.2, 0.2, 0.0])
    assert np.isfinite(r["nll"][0]) and np.isposinf(r["nll"][1])
    assert np.isfinite(r["occ"]).all() and not r["occ"][:, 1].any() and not r["occ"][:, 0, 4].any()
    assert np.isfinite(r["smooth"]).all()                                   # a class of weight 0 is left out of the sum
    bad = cr.ctc_loss_ref(lp, np.array([[1, 5, 1, 1], [1, 0, 1, 1]]), [4, 4])
    assert np.isnan(bad["nll"]).all() and not bad["occ"].any()
    assert np.isnan(cr.ctc_loss_ref(lp, tg, [5, -1])["nll"]).all()
    empty = cr.ctc_loss_ref(lp[:, :, :4], tg, [0, 0])
    assert np.allclose(empty["nll"], -lp[:, :, 0].sum(axis=0))              # len = 0: every step emits the blank


NEW_SYMBOLS = ("bh_ctc_loss_workspace", "bh_ctc_loss", "bh_ctc_loss_grad_workspace", "bh_ctc_loss_grad", "bh_ctc_loss_last_kernel")


def test_ctc_loss_symbols_are_declared_bound_and_exported():
    """Fails on the parent commit: the entry points do not exist there."""
    from bonito_amd import _lib
    text = open(os.path.join(ROOT, "include", "bonito_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES and hasattr(handle, name)
    assert handle.bh_abi_version() == 1
    enum = code[code.index("enum bh_ctc_loss_kernel {"):]
    table = {k: int(v) for k, v in re.findall(r"BH_CTC_LOSS_K_(\w+)\s*=\s*(\d+)", enum[:enum.index("};")])}
    assert table.pop("NONE") == 0 and sorted(table.values()) == sorted(_lib.CTC_LOSS_KERNELS)
    # every alpha_t in fp32, the 2 Lmax + 1 states rounded up to whole threads of the instance that serves Lmax
    ws = handle.bh_ctc_loss_grad_workspace
    assert ws(2, 10, 5, 0) == 2 * 10 * 1 * 4 + 512 and ws(2, 10, 5, 31) == 2 * 10 * 63 * 4 + 512
    assert ws(2, 10, 5, 32) == 2 * 10 * 66 * 4 + 512 and ws(3, 7, 2, 500) == 3 * 7 * 1004 * 4 + 512
    assert ws(1, 4100, 5, 2047) == 4100 * 4096 * 4 + 512
    assert ws(1, 10, 5, 2048) == 0 and ws(1, 10, 9, 4) == 0 and ws(1, 10, 1, 4) == 0 and ws(0, 10, 5, 4) == 0 and ws(1, 0, 5, 4) == 0
    assert handle.bh_ctc_loss_workspace(4, 100, 5, 600) == 512 and handle.bh_ctc_loss_workspace(4, 100, 5, 2048) == 0


def _call(with_grad=False, **kw):
    """bh_ctc_loss / bh_ctc_loss_grad with dummy pointers: every case below is refused in front of any device call."""
    from bonito_amd import _lib
    p = C.c_void_p(4096)
    a = dict(lp=p, lp32=1, N=3, T=20, C=5, s_t=15, s_n=5, targets=p, Lmax=8, tb=1, lens=p, sw=p, weight=None, smw=None, ws=p, nll=p,
             smooth=p, grad=p, g_t=15, g_n=5, g32=1, acc=0)
    a.update(kw)
    lib = _lib.lib()
    if with_grad:
        rc = lib.bh_ctc_loss_grad(a["lp"], a["lp32"], a["N"], a["T"], a["C"], a["s_t"], a["s_n"], a["targets"], a["Lmax"], a["tb"], a["lens"],
                                  a["sw"], a["weight"], a["smw"], a["ws"], a["nll"], a["smooth"], a["grad"], a["g_t"], a["g_n"], a["g32"],
                                  a["acc"], None)
    else:
        rc = lib.bh_ctc_loss(a["lp"], a["lp32"], a["N"], a["T"], a["C"], a["s_t"], a["s_n"], a["targets"], a["Lmax"], a["tb"], a["lens"],
                             a["sw"], a["ws"], a["nll"], a["smooth"], None)
    return rc, _lib.last_error()


@pytest.mark.parametrize("grad", [False, True], ids=["forward", "grad"])
def test_every_argument_error_is_reported_on_the_host(grad):
    who = "ctc_loss_grad" if grad else "ctc_loss"
    cases = [(dict(lp=None), "null pointer"), (dict(lens=None), "null pointer"), (dict(nll=None), "null pointer"),
             (dict(ws=None), "null pointer"), (dict(targets=None), "null pointer"),
             (dict(sw=None), "smooth_out needs smooth_w"),
             (dict(C=1), "C must be in 2..8 (got 1)"), (dict(C=9), "C must be in 2..8 (got 9)"),
             (dict(N=0), "empty problem"), (dict(T=0), "empty problem"),
             (dict(Lmax=-1), "Lmax must be in 0..2047 (got -1)"), (dict(Lmax=2048), "Lmax must be in 0..2047 (got 2048)"),
             (dict(tb=2), "targets must be int8 or int32"), (dict(tb=8), "targets must be int8 or int32"),
             (dict(lp32=2), "logp_fp32 must be 0 or 1"),
             (dict(s_t=4), "bad strides"), (dict(s_n=4), "bad strides"), (dict(s_n=0), "bad strides"), (dict(s_t=-15), "bad strides")]
    if grad:
        cases += [(dict(grad=None), "null pointer"), (dict(g32=2), "flags must be 0 or 1"), (dict(acc=-1), "flags must be 0 or 1"),
                  (dict(smw=C.c_void_p(4096), sw=None, smooth=None), "smooth_weight needs smooth_w"),
                  (dict(g_t=4), "the rows of grad overlap"), (dict(g_n=4), "the rows of grad overlap"),
                  (dict(g_t=14), "the rows of grad overlap"),           # [T][N][C]-like with rows of 15 elements needs g_t >= 15
                  (dict(g_t=5, g_n=99), "the rows of grad overlap")]    # [N][T][C]-like with T = 20 rows of 5 needs g_n >= 100
    for kw, msg in cases:
        rc, err = _call(grad, **kw)
        assert rc != 0 and err.startswith(who + ":") and msg in err, (kw, err)


def test_python_surface_argument_errors():
    from bonito_amd import _lib, decode
    from bonito_amd.ctc import Model
    from bonito_amd.nn import NoTorchCompute
    from conftest import load_ctc_fixture
    cfg, _, _, _ = load_ctc_fixture()
    model = Model(cfg)
    T, N, Cn = 12, 2, 5
    lp = torch.log_softmax(torch.zeros(T, N, Cn), dim=-1)
    tg, ln = torch.ones(N, 4, dtype=torch.int64), torch.tensor([4, 2])
    for fn in (decode.ctc_nll, decode.ctc_nll_grad):
        with pytest.raises(_lib.HipEngineError):                            # no CPU path
            fn(lp, tg, ln)
        with pytest.raises(ValueError, match="2..8 classes"):
            fn(torch.zeros(T, N, 9), tg, ln)
        with pytest.raises(ValueError, match="target rows"):
            fn(torch.zeros(T, 3, Cn), tg, ln)
        with pytest.raises(ValueError, match="exceed the supported 2047"):
            fn(lp, torch.ones(N, 2048, dtype=torch.int8), ln)
        with pytest.raises(TypeError, match="integers"):
            fn(lp, tg.float(), ln)
        with pytest.raises(ValueError, match="layout"):
            fn(lp, tg, ln, layout="CNT")
    with pytest.raises(_lib.HipEngineError):
        model.loss(lp, tg, ln)
    with pytest.raises(NoTorchCompute):
        model.loss(lp.clone().requires_grad_(True), tg, ln)
    with pytest.raises(NoTorchCompute):
        decode.ctc_nll(lp.clone().requires_grad_(True), tg, ln)
    with pytest.raises(ValueError, match="reduction"):
        model.ctc_label_smoothing_loss(lp, tg, ln, reduction="sum")
    assert "TRUE derivative" in Model.ctc_label_smoothing_loss.__doc__ and "TRUE DERIVATIVE" in decode.ctc_nll_grad.__doc__

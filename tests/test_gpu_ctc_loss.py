"""The CTC loss of bonito.ctc on the device (-m gpu): bh_ctc_loss / bh_ctc_loss_grad, decode.ctc_nll / ctc_nll_grad, Model.loss with
its autograd, and `python -m bonito_amd evaluate` on a bonito.ctc model directory.

TRUTH is torch's CPU fp64 ctc_loss on the very values the kernel reads (fp16 log_probs: the fp16-rounded values), which
tests/test_ctc_loss_cpu.py pins to the restatement tests/ctc_loss_ref.py and to the reference's own recorded run. torch's backward
returns exp(lp) - occ, so the occupancy is exp(lp) - grad; the kernel returns the true derivative -occ (see bh_ctc_loss_grad).

TOLERANCE. Nothing is fixed in advance, as in tests/test_gpu_seqdist_grad.py. On the SAME inputs torch's CPU ctc_loss is run in fp32 - the
reference's own arithmetic - and compared with its fp64 run: g32 = the largest absolute distance over the finite chunks of the case, of
the per-chunk loss and of the occupancy (after removing exp(lp)). The kernel is allowed, per element,
    4 x g32                                    it sums in another order and uses the hardware exp / log
  + 2^-30 x states x |weight|                  gradient only: the fixed-point combine; states = how many states of the chunk have the class
  + 2^-11 |v| + 2^-24  (fp16 output)  or  2^-23 |v|  (fp32 output)        the rounding of the written value v.
(At len = 0 torch's fp32 run subtracts the very sum it added: every occupancy is exactly 1 and g32 of the occupancy is 1e-16. The bound
is then the rounding of the written value and the fixed-point step alone; it is not widened.)
smooth is summed in fp64 by the kernel and rounded once: 2^-23 |v| against the fp64 sum of the same values.
Every test prints g32 and the kernel's distance; the measured figures are recorded in DESIGN.md section 6."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, build_ctc_model, load_ctc_fixture
import ctc_loss_ref as cr
from bonito_amd import _lib, decode

pytestmark = pytest.mark.gpu

CASES = ["t40_c2", "t48_c5", "t48_inf"]


def _rounding(v, dtype):
    v = np.abs(v)
    return 2.0 ** -11 * v + 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -23 * v


def _torch_run(lp, targets, lengths, dtype):
    """torch CPU ctc_loss on lp [T, N, C] (values as given) in `dtype` -> (nll [N], occ [T, N, C]) as float64 arrays; chunks without an
    alignment: nll = +inf and occ = 0 (zero_infinity only replaces their NaN gradient, the finite chunks are untouched)."""
    x = lp.to(dtype).clone().requires_grad_(True)
    T, N, _ = x.shape
    if targets.shape[1] == 0:
        targets = torch.zeros(N, 1, dtype=torch.int64)                       # (torch wants a column; every length is 0)
    tl = torch.full((N,), T, dtype=torch.int64)
    nll = F.ctc_loss(x, targets.long(), tl, lengths.long(), reduction="none")
    F.ctc_loss(x, targets.long(), tl, lengths.long(), reduction="sum", zero_infinity=True).backward()
    fin = torch.isfinite(nll)
    occ = (x.detach().exp() - x.grad) * fin[None, :, None]
    return nll.detach().double().numpy(), occ.double().numpy()


def _states(targets, lengths, Cn):
    """[N, C]: how many states of the chunk's blank-extended target have the class"""
    tg, ln = np.asarray(targets), np.asarray(lengths)
    out = np.zeros((len(ln), Cn))
    for n in range(len(ln)):
        out[n, 0] = ln[n] + 1
        out[n, 1:] = np.bincount(tg[n, :ln[n]].astype(np.int64), minlength=Cn)[1:Cn]
    return out


def _truth(lp, targets, lengths, weights=None):
    """One case with its references, computed once: fp64 truth, g32 of loss and occupancy, the fixed-point share, smooth."""
    nll64, occ64 = _torch_run(lp, targets, lengths, torch.float64)
    nll32, occ32 = _torch_run(lp, targets, lengths, torch.float32)
    fin = np.isfinite(nll64)
    assert (np.isfinite(nll32) == fin).all()
    c = {"nll": nll64, "occ": occ64, "fin": fin, "states": _states(targets, lengths, lp.shape[2]),
         "g32_loss": float(np.abs(nll32[fin] - nll64[fin]).max()) if fin.any() else 0.0,
         "g32_occ": float(np.abs(occ32[:, fin] - occ64[:, fin]).max()) if fin.any() else 0.0}
    if weights is not None:
        w = np.asarray(weights, np.float32).astype(np.float64)
        c["smooth"] = (lp.double().numpy()[:, :, w != 0] * w[w != 0]).sum(axis=(0, 2))
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)                                          # shared among the tests: left unchanged
    return c


def _check(tag, c, nll, grad, gdtype, weight=None, base=None, smooth=None, smooth_term=None):
    """nll [N] and grad [T, N, C] (numpy, float64) against the truth `c` under the documented bound; prints g32 and the distances."""
    fin = c["fin"]
    N = len(fin)
    w = np.ones(N) if weight is None else np.asarray(weight, np.float64)
    assert np.isposinf(nll[~fin]).all()
    dl = float(np.abs(nll[fin] - c["nll"][fin]).max()) if fin.any() else 0.0
    assert (np.abs(nll[fin] - c["nll"][fin]) <= 4 * c["g32_loss"] + 2.0 ** -23 * np.abs(c["nll"][fin])).all(), (tag, dl, c["g32_loss"])
    want = -c["occ"] * w[None, :, None]
    if smooth_term is not None:
        want = want + smooth_term * fin[None, :, None]
    err = (4 * c["g32_occ"] + 2.0 ** -30 * c["states"][None, :, :]) * np.abs(w)[None, :, None]
    if base is not None:                                                     # accumulate: the written value is base + gradient
        want = want + base
    bound = err + _rounding(want, gdtype)
    dk = float(np.abs(grad - want).max())
    print("%s: g32 loss %.3e occ %.3e | kernel loss %.3e grad %.3e" % (tag, c["g32_loss"], c["g32_occ"], dl, dk))
    assert np.isfinite(grad).all()
    if base is None:
        assert not grad[:, ~fin].any()                                       # no alignment: exactly zero
    else:
        assert (grad[:, ~fin] == base[:, ~fin]).all()                        # ... or nothing added
    assert (np.abs(grad - want) <= bound).all(), (tag, dk, c["g32_occ"])
    if smooth is not None:
        ds = float(np.abs(smooth - c["smooth"]).max())
        print("%s: smooth distance %.3e of %.3e" % (tag, ds, float(np.abs(c["smooth"]).max())))
        assert (np.abs(smooth - c["smooth"]) <= 2.0 ** -23 * np.abs(c["smooth"])).all(), (tag, ds)


@functools.lru_cache(maxsize=None)
def _fixture(name, half):
    z = np.load(os.path.join(GOLDEN, "ctc_loss.npz"))
    c = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(name + "/")}
    lp = torch.log_softmax(torch.from_numpy(c["logits"]), dim=-1)            # what the reference was given
    c["lp"] = lp.half() if half else lp
    c["tg"], c["ln"] = torch.from_numpy(c["targets"]), torch.from_numpy(c["lengths"])
    c["w"] = cr.default_weights(lp.shape[2]).astype(np.float32)
    c["truth"] = _truth(c["lp"], c["tg"], c["ln"], c["w"])
    return c


@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", CASES)
def test_fixture_nll_smooth_and_gradient(name, half):
    """fp16 / fp32 log_probs, int8 / int32 / int64 targets, both stride orders, host / device lengths, accumulate 0 and 1, the chunks
    without an alignment (+inf loss, exactly zero gradient rows). Measured on MI355X: DESIGN.md section 6."""
    c = _fixture(name, half)
    t = c["truth"]
    if name == "t48_inf":
        assert t["fin"].any() and (~t["fin"]).any()
    lp = c["lp"].cuda()
    T, N, Cn = lp.shape
    w = torch.from_numpy(c["w"])
    first = None
    for tdt, ntc, devlen in ((torch.int8, False, False), (torch.int32, True, True), (torch.int64, False, True), (torch.int64, True, False)):
        x = lp.permute(1, 0, 2).contiguous() if ntc else lp
        layout = "NTC" if ntc else "TNC"
        tg = c["tg"].to(tdt)
        ln = c["ln"].cuda() if devlen else c["ln"]
        nll0, sm0 = decode.ctc_nll(x, tg, ln, w, layout=layout)
        nll, sm, g = decode.ctc_nll_grad(x, tg, ln, w, layout=layout)
        assert g.dtype == x.dtype and g.shape == x.shape
        assert torch.equal(nll, nll0) and torch.equal(sm, sm0)               # the forward entry computes the same bits
        gt = g.permute(1, 0, 2) if ntc else g
        if first is None:
            first = (nll.clone(), sm.clone(), gt.clone())
        else:                                                                # target type, layout and the place of the lengths change nothing
            assert torch.equal(nll, first[0]) and torch.equal(sm, first[1]) and torch.equal(gt, first[2])
        _check("%s %s %s %s" % (name, "fp16" if half else "fp32", str(tdt)[6:], layout), t, nll.double().cpu().numpy(),
               gt.double().cpu().numpy(), x.dtype, smooth=sm.double().cpu().numpy())
    # per-chunk weights, the smoothing term and accumulate = 1 into an fp32 tensor that already holds something
    gen = torch.Generator().manual_seed(5)
    weight = torch.tensor([0.75, -1.25, 2.0, 1.0, 0.5, 0.25][:N])
    smw = torch.tensor([-0.5, 0.25, 1.0, 2.0, -1.0, 0.125][:N])
    base = torch.randn(T, N, Cn, generator=gen).cuda()
    out = base.clone()
    nll, sm, g = decode.ctc_nll_grad(lp, c["tg"], c["ln"], w, weight=weight, smooth_weight=smw, out=out, accumulate=True, layout="TNC")
    assert g is out and torch.equal(nll, first[0])
    term = smw.double().numpy()[None, :, None] * c["w"].astype(np.float64)[None, None, :]
    _check("%s accumulate" % name, t, nll.double().cpu().numpy(), out.double().cpu().numpy(), torch.float32, weight=weight.numpy(),
           base=base.double().cpu().numpy(), smooth_term=term)
    with pytest.raises(ValueError, match="accumulate"):
        decode.ctc_nll_grad(lp, c["tg"], c["ln"], accumulate=True)
    nll2, sm2 = decode.ctc_nll(lp, c["tg"], c["ln"])                         # without weights: no smooth
    assert sm2 is None and torch.equal(nll2, first[0])


def test_minus_infinity_log_probs_give_no_nan():
    """A class whose log-prob is -inf everywhere: the states it makes unreachable contribute occupancy 0, a target that needs the class
    has nll = +inf and a zero gradient. Truth: the restatement (torch yields NaN there); g32 = its fp32 run against its fp64 run."""
    rng = np.random.default_rng(3)
    T, N, Cn = 24, 3, 5
    x = rng.normal(size=(T, N, Cn)) * 1.5
    x[:, :, 4] = -np.inf
    lp = torch.log_softmax(torch.from_numpy(x).float(), dim=-1)
    assert torch.isneginf(lp[:, :, 4]).all()
    tg = torch.tensor([[1, 2, 3, 1, 1, 2], [1, 4, 2, 0, 0, 0], [3, 3, 3, 2, 0, 0]], dtype=torch.int8)
    ln = torch.tensor([6, 3, 4], dtype=torch.int32)
    w = np.array([0.4, 0.2, 0.2, 0.2, 0.0], np.float32)
    r64 = cr.ctc_loss_ref(lp.double().numpy(), tg.numpy(), ln.numpy(), w)
    r32 = cr.ctc_loss_ref(lp.numpy(), tg.numpy(), ln.numpy(), dtype=np.float32)
    fin = np.isfinite(r64["nll"])
    assert fin.tolist() == [True, False, True]
    t = {"nll": r64["nll"], "occ": r64["occ"], "fin": fin, "states": _states(tg, ln, Cn), "smooth": r64["smooth"],
         "g32_loss": float(np.abs(r32["nll"][fin].astype(np.float64) - r64["nll"][fin]).max()),
         "g32_occ": float(np.abs(r32["occ"].astype(np.float64) - r64["occ"]).max())}
    assert t["g32_loss"] > 0 and t["g32_occ"] > 0
    nll, sm, g = decode.ctc_nll_grad(lp.cuda(), tg, ln, torch.from_numpy(w))
    assert not g[:, :, 4].any()
    _check("-inf column", t, nll.double().cpu().numpy(), g.double().cpu().numpy(), torch.float32, smooth=sm.double().cpu().numpy())


def test_device_side_argument_errors_give_nan_and_write_nothing():
    """Lengths on the device cannot be checked on the host: len > Lmax, len < 0 or a label outside 1..C-1 give nll = NaN, and no
    element of that chunk's gradient is written; the other chunks are computed."""
    T, N, Cn = 20, 4, 5
    lp = torch.log_softmax(torch.randn(T, N, Cn, generator=torch.Generator().manual_seed(1)), dim=-1).cuda()
    tg = torch.tensor([[1, 2, 3, 4], [1, 5, 1, 1], [1, 2, 0, 0], [1, 1, 1, 1]], dtype=torch.int32)
    ln = torch.tensor([4, 4, 5, -1], dtype=torch.int32).cuda()
    out = torch.full((T, N, Cn), 7.0, device="cuda")
    nll, _, g = decode.ctc_nll_grad(lp, tg, ln, out=out)
    nll = nll.cpu().numpy()
    assert np.isfinite(nll[0]) and np.isnan(nll[1:]).all()
    assert (out[:, 1:] == 7.0).all() and not (out[:, 0] == 7.0).any()
    with pytest.raises(ValueError, match="target lengths must lie in 0..4"):
        decode.ctc_nll(lp, tg, ln.cpu())                                     # host lengths are refused before the launch


SWEEP = [(0, 5), (1, 5), (2, 5), (31, 5), (32, 5), (33, 5), (63, 5), (64, 5), (127, 5), (128, 5), (129, 5), (255, 5), (256, 5), (511, 5),
         (512, 5), (1023, 5), (2047, 5), (5, 2), (40, 8), (300, 8)]


def _instance(Lmax):
    return min(code for code, cap in _lib.CTC_LOSS_KERNELS.items() if Lmax <= cap)


@pytest.mark.parametrize("length,Cn", SWEEP, ids=["len%d_c%d" % s for s in SWEEP])
def test_length_sweep_at_the_edges_of_every_instance(length, Cn):
    """T = 2 len + 2, N = 2 (1 at len 2047), fp32 log_probs: the first and last length every instance serves, one-state-per-thread to
    sixteen, one wave and four, 2 / 5 / 8 classes (the per-thread class sums are instantiated for <= 5 and <= 8)."""
    T, N = 2 * length + 2, (1 if length == 2047 else 2)
    gen = torch.Generator().manual_seed(100 + length)
    lp = torch.log_softmax(torch.randn(T, N, Cn, generator=gen) * 2.0, dim=-1)
    tg = torch.randint(1, Cn, (N, length), generator=gen).to(torch.int8)
    if N == 2 and length > 2:
        tg[1, :length // 2] = tg[1, 0]                                       # a long run of repeats: needs more steps, shares one class
    ln = torch.full((N,), length, dtype=torch.int32)
    w = torch.from_numpy(cr.default_weights(Cn).astype(np.float32))
    t = _truth(lp, tg, ln, w.numpy())
    assert t["fin"][0]
    nll, sm, g = decode.ctc_nll_grad(lp.cuda(), tg, ln, w)
    assert _lib.lib().bh_ctc_loss_last_kernel() == _instance(length)
    _check("len %d C %d T %d (instance %d)" % (length, Cn, T, _instance(length)), t, nll.double().cpu().numpy(), g.double().cpu().numpy(),
           torch.float32, smooth=sm.double().cpu().numpy())


def test_the_sweep_reaches_every_instance_of_the_table():
    """The ids bh_ctc_loss_last_kernel() reports over the sweep's lengths (a two-step launch each: the id depends on Lmax alone) are
    exactly the launcher's instance table, for the forward and the gradient entry."""
    lib = _lib.lib()
    assert lib.bh_ctc_loss_last_kernel() in set(_lib.CTC_LOSS_KERNELS) | {0}
    for grad in (False, True):
        seen = set()
        for length, Cn in SWEEP:
            lp = torch.log_softmax(torch.zeros(2, 1, Cn), dim=-1).cuda()
            tg, ln = torch.ones(1, length, dtype=torch.int8), torch.tensor([min(length, 1)], dtype=torch.int32)
            (decode.ctc_nll_grad if grad else decode.ctc_nll)(lp, tg, ln)
            seen.add(lib.bh_ctc_loss_last_kernel())
        assert seen == set(_lib.CTC_LOSS_KERNELS)


def test_workload_shaped_case():
    """bonito.ctc's training shape: chunk 4000 at stride 3 -> T = 1334, targets of a few hundred bases, fp16 and fp32 log_probs."""
    T, N, Cn = 1334, 4, 5
    gen = torch.Generator().manual_seed(77)
    lp = torch.log_softmax(torch.randn(T, N, Cn, generator=gen) * 2.0, dim=-1)
    lens = [300, 450, 500, 600]
    ln = torch.tensor(lens, dtype=torch.int32)
    tg = torch.randint(1, Cn, (N, 600), generator=gen).to(torch.int8)
    tg = torch.where(torch.arange(600)[None, :] < ln[:, None], tg, torch.zeros_like(tg))
    w = torch.from_numpy(cr.default_weights(Cn).astype(np.float32))
    for x in (lp, lp.half()):
        t = _truth(x, tg, ln, w.numpy())
        assert t["fin"].all()
        nll, sm, g = decode.ctc_nll_grad(x.cuda(), tg, ln, w)
        assert _lib.lib().bh_ctc_loss_last_kernel() == 108
        _check("workload %s" % str(x.dtype)[6:], t, nll.double().cpu().numpy(), g.double().cpu().numpy(), x.dtype,
               smooth=sm.double().cpu().numpy())


SENTINEL = 12345.0


@pytest.mark.parametrize("g32", [False, True], ids=["grad16", "grad32"])
@pytest.mark.parametrize("length,tnc", [(6, True), (6, False), (300, True), (300, False)], ids=["wave_tnc", "wave_ntc", "multi_tnc", "multi_ntc"])
def test_guard_bytes_and_every_element_written(length, tnc, g32):
    """The C entry point with grad as a strided view (padded rows, padded planes) inside a sentinel-filled buffer, nll and smooth inside
    sentinel-filled buffers: the view starts from NaN and every element of it is written (accumulate = 0; one chunk has no alignment
    and gets zeros), every sentinel is intact."""
    lib = _lib.lib()
    N, Cn = 3, 5
    Tk = 2 * length - 2                                                      # the homopolymers below need 2 len - 1 steps: no alignment
    gen = torch.Generator().manual_seed(length)
    lp = torch.log_softmax(torch.randn(Tk, N, Cn, generator=gen) * 2.0, dim=-1).cuda()
    tg = (torch.arange(length)[None, :] % 4 + 1).repeat(N, 1).to(torch.int8)  # chunk 0: no repeats, needs len steps
    tg[1, :] = 1
    tg[2, :] = 2
    ln = torch.tensor([length, length, length], dtype=torch.int32)
    w = torch.from_numpy(cr.default_weights(Cn).astype(np.float32)).cuda()
    gdt = torch.float32 if g32 else torch.float16
    pad_c, pad_row = Cn + 3, 2
    if tnc:
        shape = (Tk + 2, N + pad_row, pad_c)
        big = torch.full(shape, SENTINEL, dtype=gdt, device="cuda")
        view = big[1:1 + Tk, 1:1 + N, 2:2 + Cn]
        g_t, g_n = view.stride(0), view.stride(1)
    else:
        shape = (N + 2, Tk + pad_row, pad_c)
        big = torch.full(shape, SENTINEL, dtype=gdt, device="cuda")
        view = big[1:1 + N, 1:1 + Tk, 2:2 + Cn]
        g_t, g_n = view.stride(1), view.stride(0)
    view.fill_(float("nan"))
    mask = torch.ones(shape, dtype=torch.bool, device="cuda")
    (mask[1:1 + Tk, 1:1 + N, 2:2 + Cn] if tnc else mask[1:1 + N, 1:1 + Tk, 2:2 + Cn]).fill_(False)
    outs = torch.full((2, N + 4), SENTINEL, dtype=torch.float32, device="cuda")
    nll, sm = outs[0, 2:2 + N], outs[1, 2:2 + N]
    tgd, lnd = tg.cuda(), ln.cuda()
    ws = torch.empty(lib.bh_ctc_loss_grad_workspace(N, Tk, Cn, length), dtype=torch.uint8, device="cuda")
    _lib.check(lib.bh_ctc_loss_grad(_lib.ptr(lp), 1, N, Tk, Cn, lp.stride(0), lp.stride(1), _lib.ptr(tgd), length, 1, _lib.ptr(lnd),
                                    _lib.ptr(w), None, None, _lib.ptr(ws), C.c_void_p(nll.data_ptr()), C.c_void_p(sm.data_ptr()),
                                    C.c_void_p(view.data_ptr()), g_t, g_n, int(g32), 0, _lib.stream_ptr()), "bh_ctc_loss_grad")
    torch.cuda.synchronize()
    assert (big[mask] == SENTINEL).all()
    assert not torch.isnan(view).any()
    assert (outs[:, :2] == SENTINEL).all() and (outs[:, 2 + N:] == SENTINEL).all()
    got = nll.cpu().numpy()
    assert np.isfinite(got[0]) and np.isposinf(got[1:]).all() and np.isfinite(sm.cpu().numpy()).all()
    v = view if tnc else view.permute(1, 0, 2)
    assert not v[:, 1:].any()                                                # zeros written for the chunks without an alignment
    dense = decode.ctc_nll_grad(lp, tg, ln, w.cpu(), out=torch.empty(Tk, N, Cn, dtype=gdt, device="cuda"))
    assert torch.equal(dense[0], nll) and torch.equal(dense[1], sm) and torch.equal(dense[2], v)       # the strides change nothing


@pytest.mark.parametrize("length", [24, 300], ids=["wave", "multi"])
def test_two_calls_are_bit_identical_on_a_homopolymer(length):
    """Every label state of a homopolymer gathers one class and every blank state class 0: the extreme case for the combine."""
    T, N, Cn = 2 * length + 10, 2, 5
    gen = torch.Generator().manual_seed(9)
    lp = torch.log_softmax(torch.randn(T, N, Cn, generator=gen) * 2.0, dim=-1).cuda()
    tg = torch.full((N, length), 3, dtype=torch.int8)
    tg[1, ::7] = 1
    ln = torch.full((N,), length, dtype=torch.int32)
    a = decode.ctc_nll_grad(lp, tg, ln)
    b = decode.ctc_nll_grad(lp, tg, ln)
    assert torch.isfinite(a[0]).all()
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


def test_split_of_the_batch_changes_nothing():
    """A workspace budget that holds two chunks (then one) per launch: identical to the unsplit call, bit for bit."""
    c = _fixture("t48_c5", False)
    lp = c["lp"].cuda()
    T, N, Cn = lp.shape
    w = torch.from_numpy(c["w"])
    per = _lib.lib().bh_ctc_loss_grad_workspace(1, T, Cn, c["tg"].shape[1]) - 512
    whole = decode.ctc_nll_grad(lp, c["tg"], c["ln"], w)
    for budget, layout in ((2 * per + 100, "TNC"), (1, "TNC"), (2 * per, "NTC")):
        x = lp if layout == "TNC" else lp.permute(1, 0, 2).contiguous()
        part = decode.ctc_nll_grad(x, c["tg"], c["ln"], w, layout=layout, workspace_budget=budget)
        g = part[2] if layout == "TNC" else part[2].permute(1, 0, 2)
        assert torch.equal(part[0], whole[0]) and torch.equal(part[1], whole[1]) and torch.equal(g, whole[2])


def _model():
    cfg, sd, _, _ = load_ctc_fixture()
    return build_ctc_model(cfg, sd), cfg, sd


@pytest.mark.parametrize("name", CASES)
def test_model_loss_dict_against_the_reference(name):
    """Model.loss / ctc_label_smoothing_loss: the reference's keys, and its recorded fp32 values (on fp32 and on fp16 log_probs).
    |ours - recorded| <= |ours - fp64| + |fp64 - recorded|: the first under the kernel's bound (4 x g32 of the per-chunk loss divided by
    the length, fp32 rounding of value and mean), the second is what the reference's own fp32 run is away from fp64."""
    model, _, _ = _model()
    for half, tag in ((False, "ref32"), (True, "ref16")):
        c = _fixture(name, half)
        t = c["truth"]
        T, N, Cn = c["lp"].shape
        d = model.loss(c["lp"].cuda(), c["tg"], c["ln"])
        assert list(d) == ["total_loss", "loss", "label_smooth_loss"]
        d64 = cr.loss_dict(c["lp"].double().numpy(), c["targets"], c["lengths"])
        lens = np.maximum(c["lengths"], 1)
        eps_loss = (4 * t["g32_loss"] / lens[t["fin"]]).max() + 2.0 ** -22 * abs(d64["loss"]) if t["fin"].all() else 0.0
        eps_ls = 2.0 ** -22 * abs(d64["label_smooth_loss"])
        for key, ref, eps in zip(("total_loss", "loss", "label_smooth_loss"), c[tag], (eps_loss + eps_ls, eps_loss, eps_ls)):
            got = float(d[key])
            print("%s %s %s: ours %.9g recorded %.9g fp64 %.9g" % (name, tag, key, got, ref, d64[key]))
            if np.isinf(ref):
                assert np.isposinf(got)
            else:
                assert abs(got - d64[key]) <= eps and abs(got - ref) <= eps + abs(d64[key] - ref)
        none = model.loss(c["lp"].cuda(), c["tg"], c["ln"], reduction="none")
        nll, _ = decode.ctc_nll(c["lp"].cuda(), c["tg"], c["ln"])
        assert torch.equal(none["loss"], nll / c["ln"].cuda().float().clamp(min=1)) and none["loss"].shape == (N,)
        assert torch.equal(none["total_loss"], none["loss"] + none["label_smooth_loss"])
        assert torch.equal(none["label_smooth_loss"], d["label_smooth_loss"])


@pytest.mark.parametrize("name", CASES)
def test_model_loss_backward_against_the_reference(name):
    """logits -> log_softmax (torch, on the device: test plumbing) -> Model.loss(...)['total_loss'].backward(): the gradient with respect
    to the LOGITS against torch's fp64 gradient of the reference's formula recorded in the fixture. Per element of d total / d log_probs
    the kernel's bound holds, scaled by 1 / (N len_n); log_softmax's backward g - exp(lp) sum_c g carries it through (e_c + p_c sum e) and
    adds fp32 roundings of its own terms (2^-22 of their magnitudes). A chunk without an alignment: exactly zero."""
    model, _, _ = _model()
    c = _fixture(name, False)
    T, N, Cn = c["lp"].shape
    x = torch.from_numpy(c["logits"]).cuda().requires_grad_(True)
    lp = torch.log_softmax(x, dim=-1)
    exact = lp.detach().cpu()                                                # the values the kernel reads (the device's log_softmax)
    t = _truth(exact, c["tg"], c["ln"], c["w"])
    d = model.loss(lp, c["tg"], c["ln"])
    with torch.no_grad():
        plain = model.loss(lp.detach(), c["tg"], c["ln"])
    assert all(torch.equal(d[k].detach(), plain[k]) for k in d)               # the value is bit-equal to the no-grad path
    d["total_loss"].backward()
    got = x.grad.double().cpu().numpy()
    fin = t["fin"]
    lens = np.maximum(c["lengths"], 1).astype(np.float64)
    lp64 = exact.double().numpy()
    w = c["w"].astype(np.float64)
    scale = fin / (N * lens)
    g = -t["occ"] * scale[None, :, None] - (w / (T * N * Cn))[None, None, :] * fin[None, :, None]
    want = cr.logsoftmax_projection(g, lp64)
    slack = 0.0
    if "total_grad_logits64" in c:
        # the recording starts from fp64 log_probs, the kernel from their fp32 roundings: to first order nll moves by at most
        # T x 2^-24 max|lp| ~ 5e-5 and the occupancies by that order; the distance of the two truths is measured, not assumed
        slack = float(np.abs(want - c["total_grad_logits64"]).max())
        assert slack <= 1e-4
        want = c["total_grad_logits64"]
    e = (4 * t["g32_occ"] + 2.0 ** -30 * t["states"][None, :, :]) * scale[None, :, None] + 2.0 ** -23 * np.abs(g)
    p = np.exp(lp64)
    bound = e + p * e.sum(axis=-1, keepdims=True) + 2.0 ** -22 * (np.abs(g) + p * np.abs(g).sum(axis=-1, keepdims=True)) + slack
    dk = float(np.abs(got - want).max())
    print("%s backward: g32 occ %.3e, d total / d logits vs fp64 %.3e (largest bound %.3e)" % (name, t["g32_occ"], dk, bound.max()))
    assert not got[:, ~fin].any()
    assert (np.abs(got - want) <= bound).all(), dk
    # fp16 log_probs: the gradient comes back in fp16; reduction='none' with an upstream vector
    x16 = c["lp"].half().cuda().requires_grad_(True)
    up = torch.tensor([0.75, -1.25, 2.0, 1.0, 0.5, 0.25][:N], device="cuda")
    model.loss(x16, c["tg"], c["ln"], reduction="none")["loss"].backward(up)
    t16 = _fixture(name, True)["truth"]
    want16 = -t16["occ"] * (up.double().cpu().numpy() * t16["fin"] / lens)[None, :, None]
    err = (4 * t16["g32_occ"] + 2.0 ** -30 * t16["states"][None, :, :]) * np.abs(up.cpu().numpy() / lens)[None, :, None]
    assert x16.grad.dtype == torch.float16
    assert (np.abs(x16.grad.double().cpu().numpy() - want16) <= err + 2.0 ** -23 * np.abs(want16) + _rounding(want16, torch.float16)).all()


def test_evaluate_cli_on_a_ctc_model_directory(tmp_path, capsys):
    """`python -m bonito_amd evaluate` on a bonito.ctc model directory: it used to die with an AttributeError (no decode_batch, no loss)."""
    from bonito_amd.cli import evaluate
    cfg, sd, x, _ = load_ctc_fixture()

    def tv(v):
        if isinstance(v, bool):
            return "true" if v else "false"
        if isinstance(v, str):
            return json.dumps(v)
        if isinstance(v, list):
            return "[" + ", ".join(tv(i) for i in v) + "]"
        return repr(v)

    mdir, ddir, odir = tmp_path / "model", tmp_path / "chunks", tmp_path / "out"
    mdir.mkdir(); ddir.mkdir()
    lines = []
    for section in ("model", "labels", "input", "encoder", "qscore"):
        lines.append("[%s]" % section)
        lines += ["%s = %s" % (k, tv(v)) for k, v in cfg[section].items()]
    for block in cfg["block"]:
        lines.append("[[block]]")
        lines += ["%s = %s" % (k, tv(v)) for k, v in block.items()]
    (mdir / "config.toml").write_text("\n".join(lines) + "\n")
    torch.save(sd, str(mdir / "weights_1.tar"))
    n = x.shape[0]
    assert x.shape[1:] == (1, 600)
    np.save(ddir / "chunks.npy", x[:, 0].numpy().astype(np.float32))
    rng = np.random.default_rng(2)
    lens = np.array([20, 45, 60][:n], np.uint16)
    refs = rng.integers(1, 5, size=(n, 60)).astype(np.uint8)
    for i in range(n):
        refs[i, lens[i]:] = 0
    np.save(ddir / "references.npy", refs)
    np.save(ddir / "reference_lengths.npy", lens)
    args = evaluate.argparser().parse_args([str(mdir), "--directory", str(ddir), "--weights", "1", "--chunks", str(n), "--batchsize", "2",
                                            "--output_dir", str(odir)])
    assert evaluate.main(args) == 0
    out = capsys.readouterr().out
    assert re.search(r"^\* num_chunks\s+%d$" % n, out, flags=re.M)
    acc = re.search(r"^\* accuracy\s+([0-9.]+)%$", out, flags=re.M)
    mean = re.search(r"^\* loss mean\s+([0-9.]+)$", out, flags=re.M)
    assert acc and 0.0 <= float(acc.group(1)) <= 100.0 and mean
    summ = (odir / "summ.txt").read_text().split("\n")
    assert summ[0].split("\t")[1:3] == ["loss", "accuracy"] and len(summ) == n + 2
    # the loss column is Model.loss(reduction='none') of the same forward
    model = build_ctc_model(cfg, sd).half().to("cuda")
    lp = model(x.half().cuda())
    want = model.loss(lp, torch.from_numpy(refs.astype(np.int32)), torch.from_numpy(lens.astype(np.int32)), reduction="none")["loss"]
    got = np.array([float(row.split("\t")[1]) for row in summ[1:1 + n]])
    # (the command ran batches of 2 and 1, this forward one of 3: the engine may pick other GEMM instances, and its log-probs are fp16,
    # 2^-11 relative each; summ.txt prints six decimals)
    assert np.isfinite(got).all() and (np.abs(got - want.cpu().numpy()) <= 2.0 ** -9 * np.abs(got) + 1e-6).all()
    assert float(mean.group(1)) == pytest.approx(got.mean(), abs=1e-4)
    rows = (odir / "refs.fasta").read_text().split("\n")[1::2][:n]
    assert rows == ["".join("NACGT"[c] for c in refs[i, :lens[i]]) for i in range(n)]

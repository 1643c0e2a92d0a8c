"""tests/attention_train_ref.py pinned on the CPU - the written-out backward against fp64 autograd and central differences, the bound
4 d16 against planted defects, the probe sweep of tests/attention_train_cases.py (decisive for every case, and the four window defects
rejected at the widest windows) - and the host side of the training attention layer: what bonito_amd.attn and the library refuse without
a device, and that header, binding and library agree on the bh_attention_train_* entries."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import attention_ref as ar
import attention_train_cases as tc
import attention_train_ref as tr
from bonito_amd import _lib, attn
from bonito_amd.nn import NoTorchCompute
from bonito_amd.transformer.model import MultiHeadAttention

SYMBOLS = ("bh_attention_train_saved_bytes", "bh_attention_train_backward_workspace", "bh_attention_train_forward",
           "bh_attention_train_backward")
DEFECT_SHAPES = ((2, 40, 2, (3, 5)), (1, 150, 2, (40, 41)), (1, 300, 1, (127, 128)), (2, 130, 3, (1, 7)))      # (N, T, H, window)


@functools.lru_cache(maxsize=None)
def _exact(N, T, H, window, kind):
    qkv, dout = tr.make_case(N, T, H, kind, seed=1)
    want = tr.exact(qkv, dout, window)
    return qkv, dout, want, tr.d16(qkv, dout, window, want)


@pytest.mark.parametrize("kind", ["gauss", "peaked"])
@pytest.mark.parametrize("N,T,H,window", [(2, 40, 2, (3, 5)), (1, 70, 1, (0, 9)), (1, 33, 2, (12, 0)), (1, 17, 1, (0, 0))], ids=lambda v: str(v))
def test_written_out_backward_equals_fp64_autograd(N, T, H, window, kind):
    """Both are fp64 statements of the same derivative: they agree to rounding (1e-12 of the largest element; sums of at most
    T 64 terms). The forward is attention_ref's."""
    qkv, dout = tr.make_case(N, T, H, kind, seed=2)
    got, want = tr.exact(qkv, dout, window), tr.autograd(qkv, dout, window)
    assert np.array_equal(got[0], ar.bh_attention(qkv.astype(np.float64), window))
    for name, g, w in zip(("out",) + tr.PARTS, got, want):
        assert g.shape == w.shape, name
        if float(np.abs(w).max()) < 1e-300:
            assert float(np.abs(g).max()) < 1e-15, name            # (0, 0): dq and dk vanish
        else:
            assert tr.dist(g, w) < 1e-12, (name, tr.dist(g, w))


def test_written_out_backward_agrees_with_central_differences():
    """L = sum(out * dout) in fp64; central differences with step 1e-6, held to 1e-6 of the gradient's largest element on a sample of
    elements of q, k and v."""
    N, T, H, window = 1, 12, 1, (2, 4)
    qkv, dout = tr.make_case(N, T, H, "gauss", seed=3)
    qkv, dout = qkv.astype(np.float64), dout.astype(np.float64)
    grads = tr.exact(qkv, dout, window)[1:]
    rng = np.random.default_rng(5)
    for part, grad in enumerate(grads):
        for _ in range(6):
            t, d = int(rng.integers(T)), int(rng.integers(64))
            vals = []
            for sgn in (1.0, -1.0):
                moved = qkv.copy()
                moved[0, t, part, 0, d] += sgn * 1e-6
                vals.append(float((ar.bh_attention(moved, window) * dout).sum()))
            fd = (vals[0] - vals[1]) / 2e-6
            assert abs(fd - grad[0, t, 0, d]) <= 1e-6 * np.abs(grad).max(), (tr.PARTS[part], t, d, fd, grad[0, t, 0, d])


@pytest.mark.parametrize("kind", ["gauss", "peaked"])
@pytest.mark.parametrize("N,T,H,window", DEFECT_SHAPES, ids=lambda v: str(v))
def test_fp16_storage_is_small_and_every_planted_defect_lies_far_beyond_the_bound(N, T, H, window, kind):
    """d16 is what fp16 storage costs a correct kernel (a few 1e-4 to a few 1e-3); a kernel passes with dist <= 4 d16. Every planted
    defect moves at least one of dq, dk, dv beyond 10 x that bound. The windows are asymmetric: the mirror matters."""
    qkv, dout, want, d16 = _exact(N, T, H, window, kind)
    print("d16 %s %s: %s" % ((N, T, H, window), kind, " ".join("%s %.2e" % kv for kv in d16.items())))
    assert all(1e-5 < v < 5e-3 for v in d16.values()), d16
    for defect in tr.DEFECTS:
        got = tr.exact(qkv, dout, window, defect=defect)
        ratios = {name: tr.dist(g, w) / (4 * d16[name]) for name, g, w in zip(tr.PARTS, got[1:], want[1:])}
        print("  defect %-11s: dist / (4 d16) = %s" % (defect, " ".join("%s %.0f" % kv for kv in ratios.items())))
        assert max(ratios.values()) > 10, (defect, ratios)


@pytest.mark.parametrize("case", tc.CASES, ids=tc.case_id)
def test_probe_sweep_is_decisive_for_every_case(case):
    """What the device sweep asserts in front of every launch, without a device: 4 d16 < smallest probe effect / 10 per part; and that the
    case probes what it is there for."""
    N, T, H, window, need = case
    ref = tc.references(case)
    pr = ref["probes"]
    print("%s: %s" % (tc.case_id(case), "  ".join("%s d16 %.2e effect %.2e (%.1f x 40 d16)" % (
        p, ref["d16"][p], ref["effects"][p], ref["effects"][p] / (40 * ref["d16"][p]) if ref["d16"][p] else np.inf) for p in tr.PARTS)))
    assert tc.need_tiles(window) == need
    tc.check_decisive(tc.case_id(case), ref["d16"], ref["effects"])
    own = np.broadcast_to(np.arange(N)[:, None, None], pr["pn"].shape)
    unseen_here, unseen_there = pr["pair"] & ~pr["seen"] & (pr["pn"] == own), pr["pair"] & (pr["pn"] != own)
    assert not (pr["seen"] & (pr["pn"] != own)).any()         # a row of another chunk must never be seen
    assert unseen_here.any() or unseen_there.any()
    if case in tc.RUNG_CASES:
        t0 = tc.sweep_length(window)
        assert t0 <= T <= t0 + 15 and pr["seen"].any() and unseen_here.any()
        i, j = np.nonzero(pr["seen"])[1], pr["pt"][pr["seen"]]          # seen pairs that cross a block seam of 128, in either direction
        assert (i // 128 < j // 128).any() or window[1] == 0
        assert (i // 128 > j // 128).any() or window[0] == 0
    if case in tc.SEAM_CASES or (case in tc.EDGE_CASES and T < max(window)):
        assert N >= 3 and (pr["pn"][unseen_there] < own[unseen_there]).any() and (pr["pn"][unseen_there] > own[unseen_there]).any()


def test_probe_sweep_launches_every_rung_at_both_needs_in_every_direction():
    got = {}
    for N, T, H, (wl, wr), need in tc.RUNG_CASES:
        got.setdefault(need, set()).add("symmetric" if abs(wl - wr) <= 1 else "left" if wr == 0 else "right" if wl == 0 else "other")
    assert got == {6: {"symmetric", "left", "right"}, 7: {"symmetric", "left", "right"}, 10: {"symmetric", "left", "right"},
                   11: {"symmetric", "right"}, 18: {"symmetric", "left", "right"}, 19: {"symmetric", "left"},
                   26: {"symmetric", "left", "right"}}
    odd = sum(T % 16 != 0 for _, T, _, _, _ in tc.RUNG_CASES)
    assert len(tc.RUNG_CASES) // 3 <= odd <= 2 * len(tc.RUNG_CASES) // 3 + 1
    edges = {(T, w) for N, T, H, w, need in tc.EDGE_CASES}
    assert edges >= {(T, w) for T in (1, 17, 127, 128, 129, 257) for w in ((40, 41), (136, 137))} | {(130, (0, 0)), (130, (1, 7))}
    assert {(N, T, H, w) for N, T, H, w, need in tc.SEAM_CASES} == {(3, 129, 2, (40, 41)), (3, 144, 2, (200, 200)), (3, 130, 3, (1, 7))}
    assert all(c in tc.CASES for c in tc.PLANE_CASES)


WIDE = {(200, 200): 585, (0, 400): 1041, (400, 0): 1056}          # the widest windows, each at its length in the sweep


@pytest.mark.parametrize("window", list(WIDE), ids=lambda v: str(v))
def test_window_defects_at_the_widest_windows_fail_on_probes(window):
    """drop_left, unmirrored, drop_right_key_pass (one long chunk) and seam_leak (three chunks shorter than the window) each move a part
    beyond 10 x (4 d16) on probe inputs, in absolute terms as the device sweep judges. On Gaussian inputs the old criterion
    (max|a - exact| / max|exact| <= 4 d16 over the tensor) is printed beside it, not asserted: that figure is why the probes exist."""
    for defects, (N, T, H) in ((("drop_left", "unmirrored", "drop_right_key_pass"), (1, WIDE[window], 1)), (("seam_leak",), (3, 144, 1))):
        case = (N, T, H, window, tc.need_tiles(window))
        ref = tc.references(case)
        tc.check_decisive(tc.case_id(case), ref["d16"], ref["effects"])
        gq, gd = tr.make_case(N, T, H, "gauss", seed=1)
        gwant = tr.exact(gq, gd, window)
        gd16 = tr.d16(gq, gd, window, gwant)
        for defect in defects:
            got = tr.exact(ref["qkv"], ref["dout"], window, defect=defect)
            err = tc.errors(got[1:], ref["want"])
            ratios = {p: err[p] / (4 * ref["d16"][p]) for p in tr.PARTS}
            old = {p: tr.dist(g, w) / (4 * gd16[p]) for p, g, w in zip(tr.PARTS, tr.exact(gq, gd, window, defect=defect)[1:], gwant[1:])}
            print("%s N%d T%d %-19s probes: error / (4 d16) = %s | gauss, old criterion: dist / (4 d16) = %s -> %s" % (
                window, N, T, defect, " ".join("%s %.0f" % kv for kv in ratios.items()), " ".join("%s %.2f" % kv for kv in old.items()),
                "caught" if max(old.values()) > 1 else "NOT caught"))
            if defect == "drop_left":                         # ONE wrong pair on the Gaussian inputs (the key at -wl of one query) under the old criterion
                i = np.arange(window[0], T)
                pairs = {"pair": np.zeros((N, T, H), bool), "pn": np.zeros((N, T, H), int), "pt": np.zeros((N, T, H), int)}
                pairs["pair"][0, i, 0], pairs["pt"][0, i, 0] = True, i - window[0]
                stats = tr.exact(gq, gd, window, stats=True)
                for label, fn in (("median", np.median), ("largest", np.max)):
                    eff = tc.probe_effects(gq, gd, pairs, stats[4], stats[5], reduce=fn)
                    print("%s N%d T%d one pair at -wl, gauss, old criterion: %s effect / (4 d16 max|exact|) = %s" % (window, N, T, label, " ".join(
                        "%s %.3f" % (p, eff[p] / (4 * gd16[p] * np.abs(w).max())) for p, w in zip(tr.PARTS, gwant[1:]))))
            if defect == "unmirrored" and window[0] == window[1]:
                assert max(err.values()) == 0.0               # a symmetric window is its own mirror: nothing to catch
            else:
                assert max(ratios.values()) > 10, (defect, ratios)


def test_single_key_reference_and_bound():
    """Window (0, 0): out = v, dv = dout, dq = dk = 0 exactly, and the derived bound is positive and tiny beside the inputs."""
    qkv, dout = tr.make_case(1, 17, 1, "gauss", seed=4)
    for s16 in (False, True):
        out, dq, dk, dv = tr.exact(qkv, dout, (0, 0), storage_fp16=s16)
        assert np.array_equal(out, qkv[:, :, 2].astype(np.float64).reshape(1, 17, 64))
        assert np.array_equal(dv.reshape(1, 17, 64), dout.astype(np.float64))
        assert np.abs(dq).max() < 1e-15 and np.abs(dk).max() < 1e-15
    bq, bk = tr.single_key_bounds(qkv, dout)
    assert bq.shape == (1, 17, 1, 64) and 0 < bq.max() < 1e-3 and 0 < bk.max() < 1e-3


def test_module_yardstick_runs_on_the_cpu_and_is_close_to_exact():
    case = tr.make_mha_case(2, 40, 128, qkv_bias=True, seed=1)
    want, got = tr.mha_exact(case, 2, (3, 5)), tr.mha_yardstick(case, 2, (3, 5))
    for name, a, w in zip(tr.MHA_NAMES, got, want):
        assert 1e-9 < tr.dist(a.numpy(), w.numpy()) < 0.1, (name, tr.dist(a.numpy(), w.numpy()))
    # the restatement's attention core is the written-out one
    qkv, dout = tr.make_case(1, 24, 2, "gauss", seed=6)
    x = torch.from_numpy(qkv.astype(np.float64))
    assert tr.dist(tr._torch_attention(x, (3, 5), torch.float64).numpy(), tr.exact(qkv, dout, (3, 5))[0]) < 1e-13


def _cpu_qkv(N=2, T=5, H=2, d=64, dtype=torch.float16):
    return torch.zeros(N, T, 3, H, d, dtype=dtype)


def test_attn_refuses_cpu_tensors():
    qkv = _cpu_qkv()
    out = torch.zeros(2, 5, 128, dtype=torch.float16)
    with pytest.raises(NoTorchCompute):
        attn.attention_forward(qkv, (3, 5))
    with pytest.raises(NoTorchCompute):
        attn.attention(qkv.float(), (3, 5))
    with pytest.raises(NoTorchCompute):
        attn.attention_forward(qkv.reshape(2, 5, 384), (3, 5))
    with pytest.raises(NoTorchCompute):
        attn.attention_backward(qkv, out, torch.zeros(256, dtype=torch.uint8), out, (3, 5))
    with pytest.raises(NoTorchCompute):
        attn.mha_module(MultiHeadAttention(128, 2, attn_window=(3, 5)), torch.zeros(2, 5, 128, dtype=torch.float16))
    with pytest.raises(NoTorchCompute):                                          # the container itself still computes nothing
        MultiHeadAttention(128, 2, attn_window=(3, 5))(torch.zeros(2, 5, 128))


def test_attn_refuses_bad_dtypes_shapes_and_windows_before_any_launch():
    qkv = _cpu_qkv()
    with pytest.raises(ValueError, match="float16 or float32"):
        attn.attention(qkv.double(), (3, 5))
    with pytest.raises(ValueError, match="must be float16"):
        attn.attention_forward(qkv.float(), (3, 5))
    with pytest.raises(ValueError, match="must be a tensor"):
        attn.attention_forward(qkv.numpy(), (3, 5))
    with pytest.raises(ValueError, match="head_dim 64"):
        attn.attention(_cpu_qkv(d=32), (3, 5))
    with pytest.raises(ValueError, match="head_dim 64"):
        attn.attention(torch.zeros(2, 5, 3 * 2 * 32 + 64, dtype=torch.float16), (3, 5))
    with pytest.raises(ValueError, match=r"\[N\]\[T\]\[3\]\[H\]\[64\]"):
        attn.attention(qkv[0], (3, 5))
    with pytest.raises(ValueError, match=r"\[N\]\[T\]\[3\]\[H\]\[64\]"):
        attn.attention(torch.zeros(2, 5, 2, 2, 64, dtype=torch.float16), (3, 5))
    with pytest.raises(ValueError, match="at least 1"):
        attn.attention(qkv[:, :0], (3, 5))
    for window in ((-1, -1), (-1, 5), (3, -2)):
        with pytest.raises(ValueError, match="finite window"):
            attn.attention(qkv, window)
    for window in ((200, 201), (0, 401), (1 << 30, 1 << 30)):
        with pytest.raises(ValueError, match="too wide"):
            attn.attention_forward(qkv, window)
    with pytest.raises(ValueError, match=r"\(left, right\)"):
        attn.attention(qkv, 5)
    assert attn.supported_window((200, 200)) and attn.supported_window((0, 400)) and not attn.supported_window((0, 401))
    assert not attn.supported_window((-1, -1)) and not attn.supported_window(None)


def test_mha_module_refuses_what_the_kernels_do_not_serve():
    x = torch.zeros(2, 5, 128, dtype=torch.float16)
    with pytest.raises(ValueError, match="MultiHeadAttention container"):
        attn.mha_module(torch.nn.MultiheadAttention(128, 2), x)
    with pytest.raises(ValueError, match="head_dim 64"):
        attn.mha_module(MultiHeadAttention(128, 4, attn_window=(3, 5)), x)
    with pytest.raises(ValueError, match="rotary_dim"):
        attn.mha_module(MultiHeadAttention(128, 2, rotary_dim=32, attn_window=(3, 5)), x)
    with pytest.raises(ValueError, match="finite window"):
        attn.mha_module(MultiHeadAttention(128, 2), x)                           # attn_window None = (-1, -1)
    with pytest.raises(ValueError, match="too wide"):
        attn.mha_module(MultiHeadAttention(128, 2, attn_window=(300, 300)), x)
    with pytest.raises(ValueError, match=r"\[N\]\[T\]\[128\]"):
        attn.mha_module(MultiHeadAttention(128, 2, attn_window=(3, 5)), x[:, :, :64])


def test_library_refuses_without_a_launch():
    """The argument checks sit in front of every device call (the pointers below are never read)."""
    lib = _lib.lib()
    N, T, H = 2, 40, 3
    assert lib.bh_attention_train_saved_bytes(N, T, H) >= N * T * H * 4
    assert lib.bh_attention_train_saved_bytes(0, T, H) == 0 and lib.bh_attention_train_saved_bytes(N, 0, H) == 0
    assert lib.bh_attention_train_saved_bytes(N, T, 0) == 0 and lib.bh_attention_train_saved_bytes(65536, T, H) == 0
    assert lib.bh_attention_train_backward_workspace(N, T, H, 3, 5) >= N * T * H * 4
    assert lib.bh_attention_train_backward_workspace(N, T, H, 200, 200) > 0
    for wl, wr in ((-1, -1), (200, 201), (-1, 5), (1 << 30, 1 << 30)):
        assert lib.bh_attention_train_backward_workspace(N, T, H, wl, wr) == 0
    assert lib.bh_attention_train_backward_workspace(0, T, H, 3, 5) == 0
    p = C.c_void_p(4096)
    big = 1 << 30

    def fwd(N=N, T=T, H=H, hd=64, wl=3, wr=5, qkv=p, saved_bytes=big):
        return lib.bh_attention_train_forward(qkv, p, N, T, H, hd, wl, wr, p, p, saved_bytes, None)

    def bwd(N=N, T=T, H=H, hd=64, wl=3, wr=5, qkv=p, ws_bytes=big):
        return lib.bh_attention_train_backward(qkv, p, p, p, p, N, T, H, hd, wl, wr, p, p, ws_bytes, None)

    for call in (fwd, bwd):
        assert call(hd=32) != 0 and "only head_dim 64" in _lib.last_error()
        assert call(wl=-1, wr=-1) != 0 and "finite window" in _lib.last_error()
        assert call(wl=3, wr=-5) != 0 and "finite window" in _lib.last_error()
        assert call(wl=200, wr=201) != 0 and "too wide" in _lib.last_error()
        assert call(T=0) != 0 and "must be positive" in _lib.last_error()
        assert call(N=65536) != 0 and "at most 65535" in _lib.last_error()
        assert call(qkv=None) != 0 and "null pointer" in _lib.last_error()
        assert call(qkv=C.c_void_p(4104)) != 0 and "16-byte aligned" in _lib.last_error()
    assert fwd(saved_bytes=lib.bh_attention_train_saved_bytes(N, T, H) - 1) != 0 and "saved buffer" in _lib.last_error()
    assert bwd(ws_bytes=16) != 0 and "workspace of 16 bytes" in _lib.last_error()
    assert lib.bh_abi_version() == 1


def test_header_binding_and_exports_agree_for_the_training_entries():
    text = open(os.path.join(ROOT, "include", "bonito_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = _lib.lib()
    for name in SYMBOLS:
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert m, "include/bonito_hip.h does not declare %s" % name
        assert name in _lib.SIGNATURES and hasattr(handle, name)
        n_args = len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])
        assert n_args == len(_lib.SIGNATURES[name][1]), name
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("bh_attention_train_")) == sorted(SYMBOLS)
    assert set(attn.__all__) >= {"attention_forward", "attention_backward", "attention", "mha_module"}

"""tests/lstm_train_ref.py pinned on the CPU - the written-out backward recurrence against fp64 autograd and against central finite
differences - and the host side of the training LSTM layer: what bonito_amd.rnn refuses without a device, and that header, binding and
library agree on the bh_lstm_train_* entries."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
import lstm_ref as lr
import lstm_train_ref as tr
from bonito_amd import _lib, rnn
from bonito_amd.nn import NoTorchCompute

SYMBOLS = ("bh_lstm_train_saved_bytes", "bh_lstm_train_forward", "bh_lstm_train_backward_workspace", "bh_lstm_train_backward",
           "bh_lstm_train_workgroups")


@pytest.mark.parametrize("reverse", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("cls,T,N,H", [("typical", 9, 3, 32), ("zeros", 5, 2, 32), ("long_memory", 12, 2, 32), ("saturating", 6, 3, 32),
                                       ("typical", 1, 4, 32)], ids=lambda v: str(v))
def test_written_out_recurrence_equals_fp64_autograd(cls, T, N, H, reverse):
    """Both are fp64 statements of the same derivative: they agree to rounding (1e-12 of the largest element; fp64 sums of at most
    T N 4H = 3500 terms of size <= max|.| err by ~1e-13 of it). With and without a bias (class zeros has none), at T = 1."""
    x, w_ih, w_hh, bias = lr.make_case(cls, T, N, H, seed=3)
    dh = tr.make_dh(T, N, H, seed=1)
    h, *got = tr.written_out(x, w_ih, w_hh, bias, dh, reverse)
    want = tr.exact(x, w_ih, w_hh, bias, dh, reverse)
    assert torch.equal(h, lr.free_running(x, w_ih, w_hh, bias, reverse)) or tr.dist(h, lr.free_running(x, w_ih, w_hh, bias, reverse)) < 1e-14
    for name, g, w in zip(tr.NAMES, got, want):
        if w is None:
            assert g is None and bias is None and name == "db"
            continue
        assert g.shape == w.shape
        if float(w.abs().max()) == 0.0:
            assert float(g.abs().max()) == 0.0, name
        else:
            assert tr.dist(g, w) < 1e-12, (name, tr.dist(g, w))
    if cls == "zeros":
        assert float(got[1].abs().max()) == 0.0 and float(got[2].abs().max()) == 0.0          # x = 0 and h = 0
    if T == 1:
        assert float(got[2].abs().max()) == 0.0                                                 # h_0 = 0


def test_written_out_recurrence_agrees_with_central_differences():
    """L = sum(h * dh) in fp64; central differences with step 1e-6 err by ~1e-12 / 1e-6 + 1e-12 L''' - held to 1e-6 of the gradient's
    largest element, on a sample of elements of every gradient."""
    T, N, H = 5, 2, 32
    x, w_ih, w_hh, bias = lr.make_case("typical", T, N, H, seed=5)
    dh = tr.make_dh(T, N, H, seed=2).double()
    _, dx, dwi, dwh, db = tr.written_out(x, w_ih, w_hh, bias, dh, True)
    args = [x.double(), w_ih.double(), w_hh.double(), bias.double()]
    eps = 1e-6
    g = torch.Generator().manual_seed(11)
    for k, grad in enumerate((dx, dwi, dwh, db)):
        flat = grad.reshape(-1)
        for e in torch.randint(0, flat.numel(), (6,), generator=g).tolist():
            vals = []
            for sgn in (1.0, -1.0):
                moved = [a.clone() for a in args]
                moved[k].view(-1)[e] += sgn * eps
                vals.append(float((lr.free_running(*moved, reverse=True) * dh).sum()))
            fd = (vals[0] - vals[1]) / (2 * eps)
            assert abs(fd - float(flat[e])) <= 1e-6 * float(flat.abs().max()), (tr.NAMES[k], e, fd, float(flat[e]))


def test_yardstick_runs_on_the_cpu_and_is_close_to_exact():
    """torch.nn.LSTM(H, H).half() with its autograd runs on the CPU; its distance from `exact` is that of half-precision arithmetic:
    above fp64 rounding, below ten percent."""
    for reverse in (False, True):
        x, w_ih, w_hh, bias = lr.make_case("typical", 7, 3, 32, seed=2)
        dh = tr.make_dh(7, 3, 32)
        want, got = tr.exact(x, w_ih, w_hh, bias, dh, reverse), tr.yardstick(x, w_ih, w_hh, bias, dh, reverse)
        for name, a, w in zip(tr.NAMES, got, want):
            assert 1e-9 < tr.dist(a, w) < 0.1, (name, tr.dist(a, w))


def _cpu_case(H=32, T=3, N=2, x_dtype=torch.float16, w_dtype=torch.float32):
    return torch.zeros(T, N, H, dtype=x_dtype), torch.zeros(4 * H, H, dtype=w_dtype), torch.zeros(4 * H, H, dtype=w_dtype)


def test_rnn_refuses_cpu_tensors():
    x, wi, wh = _cpu_case()
    for fn in (rnn.lstm, rnn.lstm_forward):
        with pytest.raises(NoTorchCompute):
            fn(x, wi, wh)
        with pytest.raises(NoTorchCompute):
            fn(x, wi, wh, torch.zeros(128), reverse=True)
    with pytest.raises(NoTorchCompute):
        rnn.lstm_backward(x, wi, wh, x, torch.zeros(16, dtype=torch.uint8), x)
    from bonito_amd.nn import LSTM
    with pytest.raises(NoTorchCompute):
        rnn.lstm_module(LSTM(32, 32, reverse=True), x)
    with pytest.raises(NoTorchCompute):                                          # the containers themselves still compute nothing
        LSTM(32, 32)(x)


def test_rnn_refuses_bad_dtypes_and_shapes_before_any_launch():
    x, wi, wh = _cpu_case()
    with pytest.raises(ValueError, match="float16 or float32"):
        rnn.lstm(x.double(), wi, wh)
    with pytest.raises(ValueError, match="float16"):
        rnn.lstm_forward(x.float(), wi, wh)
    with pytest.raises(ValueError, match="w_ih must be float32"):
        rnn.lstm(x, wi.half(), wh)
    with pytest.raises(ValueError, match="w_hh must be"):
        rnn.lstm(x, wi, wh[:, :16])
    with pytest.raises(ValueError, match="bias must be float32"):
        rnn.lstm(x, wi, wh, torch.zeros(64))
    with pytest.raises(ValueError, match=r"\[T\]\[N\]\[H\]"):
        rnn.lstm(x[0], wi, wh)
    for H in (48, 1056, 16):
        x, wi, wh = _cpu_case(H=H)
        with pytest.raises(ValueError, match="hidden size %d is not supported" % H):
            rnn.lstm(x, wi, wh)
    with pytest.raises(ValueError, match="bonito_amd.nn.LSTM"):
        rnn.lstm_module(torch.nn.LSTM(32, 32), x)


def test_library_refuses_without_a_launch():
    """The argument checks sit in front of every device call (the pointers below are never read)."""
    lib = _lib.lib()
    assert lib.bh_lstm_train_saved_bytes(4, 5, 48) == 0 and lib.bh_lstm_train_saved_bytes(4, 5, 1056) == 0
    assert lib.bh_lstm_train_saved_bytes(0, 5, 32) == 0 and lib.bh_lstm_train_backward_workspace(4, 0, 32) == 0
    assert lib.bh_lstm_train_backward_workspace(4, 5, 48) == 0
    T, N, H = 4, 5, 32
    rows = T * N
    # the layout the header states: gates fp16 [T][N][4H], c fp32 [T][N][H], two fp16 weight matrices (each rounded up to 256 bytes)
    assert lib.bh_lstm_train_saved_bytes(T, N, H) >= rows * 4 * H * 2 + rows * H * 4 + 2 * 4 * H * H * 2
    assert lib.bh_lstm_train_workgroups(1) == 1 and lib.bh_lstm_train_workgroups(16) == 1 and lib.bh_lstm_train_workgroups(17) == 2
    assert lib.bh_lstm_train_workgroups(64) == 4
    p = C.c_void_p(4096)
    for H_bad in (48, 1056):
        assert lib.bh_lstm_train_forward(p, p, p, None, T, N, H_bad, 0, p, p, 1 << 30, None) != 0
        assert "hidden size %d is not supported" % H_bad in _lib.last_error()
        assert lib.bh_lstm_train_backward(p, p, p, p, p, p, T, N, H_bad, 0, p, p, p, None, p, 1 << 30, None) != 0
        assert "hidden size %d is not supported" % H_bad in _lib.last_error()
    assert lib.bh_lstm_train_forward(p, p, p, None, T, N, H, 0, p, p, lib.bh_lstm_train_saved_bytes(T, N, H) - 1, None) != 0
    assert "saved buffer" in _lib.last_error()
    assert lib.bh_lstm_train_backward(p, p, p, p, p, p, T, N, H, 0, p, p, p, None, p, 16, None) != 0
    assert "workspace of 16 bytes" in _lib.last_error()
    assert lib.bh_lstm_train_forward(p, None, p, None, T, N, H, 0, p, p, 1 << 30, None) != 0 and "null pointer" in _lib.last_error()
    assert lib.bh_lstm_train_forward(p, p, p, None, 0, N, H, 0, p, p, 1 << 30, None) != 0 and "must be positive" in _lib.last_error()
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
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("bh_lstm_train_")) == sorted(SYMBOLS)
    assert set(rnn.__all__) >= {"lstm_forward", "lstm_backward", "lstm", "lstm_module"}

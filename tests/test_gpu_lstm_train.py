"""The training LSTM layer on the device (-m gpu): bh_lstm_train_forward / bh_lstm_train_backward and bonito_amd.rnn.

FORWARD. h is judged element by element against lstm_ref.teacher_forced with gemm=True (the input projection x W_ih^T + b is stored as
fp16, as the bound's `gemm` branch states it): |h - want| <= bound everywhere, no tolerance of this file's own.

BACKWARD. exact = fp64 autograd through lstm_ref.free_running; yardstick = torch.nn.LSTM(H, H).half() on the CPU with its own autograd
on the same inputs, computed live (tests/lstm_train_ref.py, pinned by tests/test_lstm_train_ref_cpu.py). With
dist(a) = max|a - exact| / max|exact|, every one of dx, dW_ih, dW_hh, db must satisfy dist(kernel) <= 2 dist(yardstick). The margin of 2
was fixed before any kernel ran: an fp32 emulation of a design that stores h, the gates and da as fp16 measured 0.02 - 1.19 of the
yardstick over these classes and shapes. Every case prints its ratios; DESIGN.md section 6 records them.

The rest is exact: zeros where the definition gives zeros, equal bytes from call to call, untouched guard bytes, a chunk's bytes
independent of the rest of the batch, refusals that launch nothing."""
import functools

import pytest
import torch

import lstm_ref as lr
import lstm_train_ref as tr
from bonito_amd import _lib, rnn
from bonito_amd.nn import LSTM

pytestmark = pytest.mark.gpu

DEV = "cuda"
MARGIN = 2.0
GRAD_CLASSES = ("typical", "long_memory", "saturating")
GRAD_SHAPES = ((37, 5, 32), (64, 16, 96), (24, 16, 384), (300, 16, 96), (4, 16, 1024), (2, 20, 32), (1, 5, 32))      # (T, N, H)


@functools.lru_cache(maxsize=None)
def _case(cls, T, N, H):
    x, w_ih, w_hh, bias = lr.make_case(cls, T, N, H, seed=1)
    return x, w_ih, w_hh, bias, tr.make_dh(T, N, H, seed=1)


@functools.lru_cache(maxsize=None)
def _references(cls, T, N, H, reverse):
    """(exact, yardstick) of a case, computed once on the CPU and never modified."""
    x, w_ih, w_hh, bias, dh = _case(cls, T, N, H)
    return tr.exact(x, w_ih, w_hh, bias, dh, reverse), tr.yardstick(x, w_ih, w_hh, bias, dh, reverse)


def _dev(t):
    return None if t is None else t.to(DEV)


@functools.lru_cache(maxsize=None)
def _device_run(cls, T, N, H, reverse):
    """-> (h, dx, dW_ih, dW_hh, db) of the kernels through bonito_amd.rnn, on the device."""
    x, w_ih, w_hh, bias, dh = (_dev(t) for t in _case(cls, T, N, H))
    h, saved = rnn.lstm_forward(x, w_ih, w_hh, bias, reverse)
    dx, dwi, dwh, db = rnn.lstm_backward(x, w_ih, w_hh, h, saved, dh, reverse, need_bias=bias is not None)
    torch.cuda.synchronize()
    return h, dx, dwi, dwh, db


@pytest.mark.parametrize("reverse", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("T,N,H", [(37, 5, 32), (64, 16, 96), (24, 16, 384), (4, 16, 1024), (150, 20, 64)], ids=lambda v: str(v))
@pytest.mark.parametrize("cls", lr.CLASSES)
def test_forward_within_the_bound_of_the_teacher_forced_reference(cls, T, N, H, reverse):
    x, w_ih, w_hh, bias, _ = (_dev(t) for t in _case(cls, T, N, H))
    h, _ = rnn.lstm_forward(x, w_ih, w_hh, bias, reverse)
    assert h.dtype == torch.float16 and tuple(h.shape) == (T, N, H)
    if cls == "zeros":
        assert int(torch.count_nonzero(h)) == 0
        return
    want, bound = lr.teacher_forced(x, w_ih, w_hh, bias, h, reverse, gemm=True)
    ratio, where = lr.worst(h, want, bound)
    print("forward %s T=%d N=%d H=%d %s: worst |h - want| / bound = %.3f at %s" % (cls, T, N, H, "rev" if reverse else "fwd", ratio, where))
    assert ratio <= 1.0


@pytest.mark.parametrize("reverse", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("T,N,H", GRAD_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("cls", GRAD_CLASSES)
def test_backward_within_twice_the_yardstick(cls, T, N, H, reverse):
    exact, yard = _references(cls, T, N, H, reverse)
    got = _device_run(cls, T, N, H, reverse)[1:]
    assert got[0].dtype == torch.float16 and all(g.dtype == torch.float32 for g in got[1:])
    if T == 1:                                                                # h_0 = 0: no row of h_prev exists
        assert int(torch.count_nonzero(got[2])) == 0
    failed = []
    for name, g, e, y in zip(tr.NAMES, got, exact, yard):
        dk, dy = tr.dist(g, e), tr.dist(y, e)
        print("backward %s T=%d N=%d H=%d %s %-5s: dist(kernel) = %.3e  dist(yardstick) = %.3e  ratio = %.3f"
              % (cls, T, N, H, "rev" if reverse else "fwd", name, dk, dy, dk / dy if dy > 0 else float("inf")))
        if not dk <= MARGIN * dy:
            failed.append((name, dk, dy))
    assert not failed, failed


@pytest.mark.parametrize("reverse", [False, True], ids=["fwd", "rev"])
def test_exact_zeros(reverse):
    """Class zeros (x = 0, no bias, hence h = 0): dW_ih and dW_hh are exactly zero; T = 1 (h_0 = 0): dW_hh is exactly zero."""
    h, dx, dwi, dwh, db = _device_run("zeros", 9, 20, 96, reverse)
    assert db is None
    assert int(torch.count_nonzero(h)) == 0 and int(torch.count_nonzero(dwi)) == 0 and int(torch.count_nonzero(dwh)) == 0
    assert int(torch.count_nonzero(dx)) > 0                                   # the gradient itself is not zero
    h, dx, dwi, dwh, db = _device_run("typical", 1, 20, 96, reverse)
    assert int(torch.count_nonzero(dwh)) == 0 and int(torch.count_nonzero(dwi)) > 0 and int(torch.count_nonzero(db)) > 0


GUARD = 512


class _Guarded:
    """A device tensor between two guard zones of GUARD bytes of 0xA5 (the payload starts 0xA5 too)."""

    def __init__(self, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        self.nbytes = n * torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((self.nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.t = self.raw[GUARD:GUARD + self.nbytes].view(dtype).view(shape)

    def guards_intact(self):
        return bool((self.raw[:GUARD] == 0xA5).all()) and bool((self.raw[GUARD + self.nbytes:] == 0xA5).all())

    def payload_untouched(self):
        return bool((self.raw == 0xA5).all())


def _raw_call(x, w_ih, w_hh, bias, dh, reverse):
    """Both entry points on buffers of this test's own -> dict of _Guarded (h, saved, dx, dw_ih, dw_hh, db)."""
    lib = _lib.lib()
    T, N, H = x.shape
    sb, wb = lib.bh_lstm_train_saved_bytes(T, N, H), lib.bh_lstm_train_backward_workspace(T, N, H)
    assert sb > 0 and wb > 0
    o = {"h": _Guarded((T, N, H), torch.float16), "saved": _Guarded((sb,), torch.uint8), "dx": _Guarded((T, N, H), torch.float16),
         "dw_ih": _Guarded((4 * H, H), torch.float32), "dw_hh": _Guarded((4 * H, H), torch.float32), "db": _Guarded((4 * H,), torch.float32)}
    ws = torch.empty(wb, dtype=torch.uint8, device=DEV)
    s = _lib.stream_ptr()
    _lib.check(lib.bh_lstm_train_forward(_lib.ptr(x), _lib.ptr(w_ih), _lib.ptr(w_hh), _lib.ptr(bias), T, N, H, int(reverse), _lib.ptr(o["h"].t),
                                         _lib.ptr(o["saved"].t), sb, s), "forward")
    _lib.check(lib.bh_lstm_train_backward(_lib.ptr(x), _lib.ptr(w_ih), _lib.ptr(w_hh), _lib.ptr(o["h"].t), _lib.ptr(o["saved"].t), _lib.ptr(dh),
                                          T, N, H, int(reverse), _lib.ptr(o["dx"].t), _lib.ptr(o["dw_ih"].t), _lib.ptr(o["dw_hh"].t),
                                          _lib.ptr(o["db"].t), _lib.ptr(ws), wb, s), "backward")
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("T,N,H,reverse", [(11, 20, 96, True), (600, 5, 32, False), (3, 37, 128, False)], ids=lambda v: str(v))
def test_two_calls_give_equal_bytes_and_guard_bytes_are_untouched(T, N, H, reverse):
    """(600, 5, 32): T N = 3000 rows, more than one partial sum of the weight gradients."""
    args = [_dev(t) for t in _case("typical", T, N, H)]
    a, b = _raw_call(*args, reverse), _raw_call(*args, reverse)
    for name in a:
        assert a[name].guards_intact() and b[name].guards_intact(), name
        if name != "saved":                                                  # (saved has alignment gaps nobody writes)
            assert torch.equal(a[name].t.view(torch.uint8), b[name].t.view(torch.uint8)), name
            assert bool(torch.isfinite(a[name].t).all()), name
    # ... and they are the bytes the public wrappers return
    h, dx, dwi, dwh, db = _device_run("typical", T, N, H, reverse)
    for name, t in (("h", h), ("dx", dx), ("dw_ih", dwi), ("dw_hh", dwh), ("db", db)):
        assert torch.equal(a[name].t, t), name


@pytest.mark.parametrize("reverse", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("N", [5, 20])
def test_tail_rows_have_the_bytes_they_have_inside_a_full_batch(N, reverse):
    """Chunks 0..N-1 alone (the last tile of 16 padded by the library) against the same chunks inside a batch of 32: h and dx."""
    T, H = 7, 96
    x, w_ih, w_hh, bias, dh = (_dev(t) for t in _case("typical", T, 32, H))
    h32, saved = rnn.lstm_forward(x, w_ih, w_hh, bias, reverse)
    dx32 = rnn.lstm_backward(x, w_ih, w_hh, h32, saved, dh, reverse)[0]
    xs, dhs = x[:, :N].contiguous(), dh[:, :N].contiguous()
    h, saved = rnn.lstm_forward(xs, w_ih, w_hh, bias, reverse)
    dx = rnn.lstm_backward(xs, w_ih, w_hh, h, saved, dhs, reverse)[0]
    assert torch.equal(h, h32[:, :N]) and torch.equal(dx, dx32[:, :N])


def test_indices_past_2_to_the_31():
    """T N 4H = 2 x 262160 x 4096 > 2^31 elements: the gate tensor, da and the partial sums are indexed with 64 bits, and the two GEMMs go
    in blocks of rows. Every chunk is the SAME chunk, so h and dx of all 262160 must have the bytes of a batch of 16, and the weight
    gradients are 16385 times those of that batch - up to the fp32 sums: one workgroup adds the T N / 32 = 16385 MFMA results of an
    element in sequence, each addition within 2^-24 relative of the running sum. The running sum grows linearly through the N equal
    terms of step 0 and then of step 1, so it never exceeds N (|a_0| + |a_1|), at most twice the largest of N |a_0| and N |a_0 + a_1|
    unless the two steps cancel; the distance is taken against the largest element, where they do not: 2 x 16385 x 2^-24 = 2e-3.
    (db: 1024 partial sums of 513 terms, far inside the same bound.)"""
    T, N, H = 2, 262160, 1024
    x1, w_ih, w_hh, bias = (_dev(t) for t in lr.make_case("typical", T, 1, H, seed=4))
    dh1 = _dev(tr.make_dh(T, 1, H, seed=4))
    small = [x1.expand(T, 16, H).contiguous(), dh1.expand(T, 16, H).contiguous()]
    h16, saved = rnn.lstm_forward(small[0], w_ih, w_hh, bias)
    dx16, dwi16, dwh16, db16 = rnn.lstm_backward(small[0], w_ih, w_hh, h16, saved, small[1])
    x, dh = x1.expand(T, N, H).contiguous(), dh1.expand(T, N, H).contiguous()
    h, saved = rnn.lstm_forward(x, w_ih, w_hh, bias)
    dx, dwi, dwh, db = rnn.lstm_backward(x, w_ih, w_hh, h, saved, dh)
    assert torch.equal(h, h16[:, :1].expand(T, N, H)) and torch.equal(dx, dx16[:, :1].expand(T, N, H))
    assert int(torch.count_nonzero(h[:, -1])) > 0 and int(torch.count_nonzero(dx[:, -1])) > 0
    bound = 2 * (T * N / 32) * 2.0 ** -24
    for name, big, sm in (("dW_ih", dwi, dwi16), ("dW_hh", dwh, dwh16), ("db", db, db16)):
        d = tr.dist(big, sm.double() * (N / 16))
        print("large %s: distance from 16385 x the batch of 16 = %.3e (bound %.3e)" % (name, d, bound))
        assert d <= bound, name


def test_a_non_finite_upstream_gradient_stays_in_its_chunk():
    T, N, H = 6, 8, 32
    x, w_ih, w_hh, bias, dh = (_dev(t) for t in _case("typical", T, N, H))
    h, saved = rnn.lstm_forward(x, w_ih, w_hh, bias, True)
    clean = rnn.lstm_backward(x, w_ih, w_hh, h, saved, dh, True)
    bad = dh.clone()
    bad[2, 3, :] = float("inf")
    dx, dwi, dwh, db = rnn.lstm_backward(x, w_ih, w_hh, h, saved, bad, True)
    others = [n for n in range(N) if n != 3]
    assert torch.equal(dx[:, others], clean[0][:, others])
    assert bool(torch.isfinite(clean[0]).all()) and not bool(torch.isfinite(dx[:, 3]).all())
    for g in (dwi, dwh, db):
        assert not bool(torch.isfinite(g).all())


def test_chain_of_two_containers_through_autograd():
    """Two nn.LSTM containers (H = 32, the second reversed) through lstm_module, then a fixed fp32 projection and a sum in torch (test
    plumbing). The first layer's three parameter gradients against the two-layer fp64 and yardstick runs, criterion as above."""
    T, N, H = 12, 6, 32
    torch.manual_seed(5)
    l1, l2 = LSTM(H, H), LSTM(H, H, reverse=True)
    with torch.no_grad():
        for layer in (l1, l2):
            for w in (layer.rnn.weight_ih_l0, layer.rnn.weight_hh_l0):
                w.copy_(w.half().float())                                   # fp16-valued weights: the same inputs for all three runs
    x = lr.make_case("typical", T, N, H, seed=9)[0]
    g = torch.Generator().manual_seed(3)
    proj = torch.randn(H, 3, generator=g)

    def params(layer):
        r = layer.rnn
        return r.weight_ih_l0.detach().clone(), r.weight_hh_l0.detach().clone(), (r.bias_ih_l0 + r.bias_hh_l0).detach().clone()

    p1, p2 = params(l1), params(l2)
    # fp64
    leaves = [p.double().requires_grad_() for p in p1]
    h1 = lr.free_running(x.double(), *leaves, reverse=False)
    h2 = lr.free_running(h1, *(p.double() for p in p2), reverse=True)
    exact = torch.autograd.grad((h2 @ proj.double()).sum(), leaves)
    # the yardstick: two half-precision torch.nn.LSTM on the CPU
    m1, m2 = tr.half_module(*p1), tr.half_module(*p2)
    y1, _ = m1(x.half())
    y2, _ = m2(y1.flip(0))
    (y2.flip(0).float() @ proj).sum().backward()
    yard = (m1.weight_ih_l0.grad, m1.weight_hh_l0.grad, m1.bias_ih_l0.grad)
    # the device
    l1.to(DEV), l2.to(DEV)
    out = rnn.lstm_module(l2, rnn.lstm_module(l1, x.to(DEV)))
    assert out.dtype == torch.float16 and out.requires_grad
    (out.float() @ proj.to(DEV)).sum().backward()
    r = l1.rnn
    assert r.bias_hh_l0.grad is None and l2.rnn.bias_hh_l0.grad is None
    got = (r.weight_ih_l0.grad, r.weight_hh_l0.grad, r.bias_ih_l0.grad)
    assert all(t is not None and t.dtype == torch.float32 for t in got) and l2.rnn.weight_hh_l0.grad is not None
    for name, a, e, y in zip(("weight_ih_l0", "weight_hh_l0", "bias_ih_l0"), got, exact, yard):
        dk, dy = tr.dist(a, e), tr.dist(y, e)
        print("chain %-12s: dist(kernel) = %.3e  dist(yardstick) = %.3e  ratio = %.3f" % (name, dk, dy, dk / dy))
        assert dk <= MARGIN * dy, name


def test_autograd_gives_gradients_only_where_they_are_asked_for():
    T, N, H = 5, 4, 32
    x, w_ih, w_hh, bias, dh = (_dev(t) for t in _case("typical", T, N, H))
    xf = x.float().requires_grad_()                                           # fp32 in: cast to fp16, its gradient comes back as fp32
    w_hh = w_hh.clone().requires_grad_()
    h = rnn.lstm(xf, w_ih, w_hh, bias, reverse=True)
    h.backward(dh)
    ref = _device_run("typical", T, N, H, True)
    assert xf.grad.dtype == torch.float32 and torch.equal(xf.grad, ref[1].float()) and torch.equal(w_hh.grad, ref[3])
    assert torch.equal(h.detach(), ref[0]) and w_ih.grad is None and bias.grad is None


def test_refusals_launch_nothing():
    lib = _lib.lib()
    T, N = 4, 5
    s = _lib.stream_ptr()
    for H in (48, 1056):
        assert lib.bh_lstm_train_saved_bytes(T, N, H) == 0 and lib.bh_lstm_train_backward_workspace(T, N, H) == 0
        x = torch.zeros(T, N, H, dtype=torch.float16, device=DEV)
        w = torch.zeros(4 * H, H, device=DEV)
        h, saved = _Guarded((T, N, H), torch.float16), _Guarded((1 << 20,), torch.uint8)
        rc = lib.bh_lstm_train_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(w), None, T, N, H, 0, _lib.ptr(h.t), _lib.ptr(saved.t), 1 << 20, s)
        assert rc != 0 and "hidden size %d is not supported" % H in _lib.last_error()
        dx, dw = _Guarded((T, N, H), torch.float16), _Guarded((4 * H, H), torch.float32)
        rc = lib.bh_lstm_train_backward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(w), _lib.ptr(x), _lib.ptr(saved.t), _lib.ptr(x), T, N, H, 0,
                                        _lib.ptr(dx.t), _lib.ptr(dw.t), _lib.ptr(dw.t), None, _lib.ptr(saved.t), 1 << 20, s)
        assert rc != 0 and "hidden size %d is not supported" % H in _lib.last_error()
        torch.cuda.synchronize()
        assert h.payload_untouched() and saved.payload_untouched() and dx.payload_untouched() and dw.payload_untouched()
        with pytest.raises(ValueError):
            rnn.lstm(x, w, w)
    H = 32
    x = torch.zeros(T, N, H, dtype=torch.float16, device=DEV)
    w = torch.zeros(4 * H, H, device=DEV)
    need = lib.bh_lstm_train_saved_bytes(T, N, H)
    h, saved = _Guarded((T, N, H), torch.float16), _Guarded((need - 256,), torch.uint8)
    rc = lib.bh_lstm_train_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(w), None, T, N, H, 0, _lib.ptr(h.t), _lib.ptr(saved.t), need - 256, s)
    assert rc != 0 and "saved buffer of %d bytes" % (need - 256) in _lib.last_error()
    torch.cuda.synchronize()
    assert h.payload_untouched() and saved.payload_untouched()

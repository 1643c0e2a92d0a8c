"""The training convolution and linear / CRF-head layer on the device (-m gpu): bh_conv1d_train_*, bh_linear_train_* and
bonito_amd.train_ops.

FORWARD. The bytes of the inference entry points (bh_conv1d_first / bh_conv1d / bh_linear with the engine's row remap) on the same
rounded weights; the device packer's bytes are bh_conv1d_pack's.

BACKWARD. exact = fp64 autograd, yardstick = the same in fp16 on the CPU, both with the clamp's mask taken from the DEVICE's own stored y
(tests/train_layers_ref.py, pinned by tests/test_train_layers_ref_cpu.py). With dist(a) = max|a - exact| / max|exact|, every one of dx,
dW, db must satisfy dist(kernel) <= 2 dist(yardstick): the project's margin for this yardstick construction (tests/test_gpu_lstm_train.py);
an fp32 emulation of the design measured 0.38 - 1.46 of the yardstick on these convolution cases and 0.0 - 1.02 on the linear cases
(tests/test_train_layers_ref_cpu.py). Every case
prints its ratios; DESIGN.md section 6 records them.

The rest is exact: zeros where the definition gives zeros, equal bytes from call to call, untouched guard bytes, a chunk's bytes
independent of the rest of the batch, null outputs honoured, refusals that launch nothing, and one linear backward past 2^31 elements."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import train_layers_ref as tl
from bonito_amd import _lib, train_ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
INF = float("inf")
CONV_VARIANTS = [(case, clamp, scale) for case in tl.CONV_CASES for clamp in (None, tl.CLAMP) for scale in (1.0, 4.0)]


def _conv_id(v):
    case, clamp, scale = v
    return "%s-%s-x%g" % ("x".join(str(c) for c in case), "clamp" if clamp else "free", scale)


def _dev(t):
    return None if t is None else t.to(DEV)


def _time_major(case):
    return case[3] == 19            # the layer in front of the LSTM stack stores [T][N][C]


@functools.lru_cache(maxsize=None)
def _conv_run(case, clamp, scale):
    """One convolution through the autograd wrapper (x as the layer sees it: [N][Lin] for one channel) -> y, dx, dw, db as [N][L][C] tensors."""
    x, w, b, dy, pad = tl.conv_inputs(case, scale)
    xd = _dev(x[:, :, 0] if case[1] == 1 else x).requires_grad_()
    wd, bd = _dev(w).requires_grad_(), _dev(b).requires_grad_()
    tm = _time_major(case)
    y = train_ops.conv1d(xd, wd, bd, case[4], pad, "swish", clamp, tm)
    y.backward(_dev(dy).permute(1, 0, 2).contiguous() if tm else _dev(dy))
    torch.cuda.synchronize()
    y = y.detach().permute(1, 0, 2) if tm else y.detach()
    dx = xd.grad[:, :, None] if case[1] == 1 else xd.grad
    return y.cpu(), dx.cpu(), wd.grad.cpu(), bd.grad.cpu()


# ---- forward ------------------------------------------------------------------------------------------------------------------------------
def _inference_conv(x, w, b, case, pad, clamp, tm):
    """bh_conv1d_first / bh_conv1d on the rounded weights and bias -> y, and the host packer's bytes (None for one input channel)."""
    N, Cin, Cout, K, stride, Lin = case
    lib = _lib.lib()
    Lout = tl.conv_out_len(Lin, K, stride, pad)
    lo, hi = clamp if clamp else (-INF, INF)
    y = torch.full((Lout, N, Cout) if tm else (N, Lout, Cout), -7.0, dtype=torch.float16, device=DEV)
    os_n, os_t = (Cout, N * Cout) if tm else (Lout * Cout, Cout)
    br = _dev(b.half().float())
    if Cin == 1:
        wr = _dev(w.half().float().contiguous())
        _lib.check(lib.bh_conv1d_first(_lib.ptr(x), _lib.ptr(wr), _lib.ptr(br), _lib.ptr(y), N, Lin, Cout, K, stride, pad, 1, lo, hi, os_n, os_t,
                                       _lib.stream_ptr()), "bh_conv1d_first")
        packed = None
    else:
        packed = np.zeros(lib.bh_conv1d_packed_halves(Cin, Cout, K), np.uint16)
        wh = np.ascontiguousarray(w.numpy())
        assert lib.bh_conv1d_pack(wh.ctypes.data_as(C.c_void_p), Cin, Cout, K, packed.ctypes.data_as(C.c_void_p)) == 0
        pk = torch.from_numpy(packed.view(np.int16)).to(DEV)
        _lib.check(lib.bh_conv1d(_lib.ptr(x), _lib.ptr(pk), _lib.ptr(br), _lib.ptr(y), N, Lin, Cin, Cout, K, stride, pad, 1, lo, hi, os_n, os_t,
                                 _lib.stream_ptr()), "bh_conv1d")
    torch.cuda.synchronize()
    return y, packed


@pytest.mark.parametrize("clamp", [None, tl.CLAMP], ids=["free", "clamp"])
@pytest.mark.parametrize("case", [c for c in tl.CONV_CASES if c[1] != 4], ids=lambda c: "x".join(str(v) for v in c))
def test_convolution_forward_has_the_bytes_of_the_inference_kernels(case, clamp):
    N, Cin, Cout, K, stride, Lin = case
    x, w, b, dy, pad = tl.conv_inputs(case)
    xd = _dev(x[:, :, 0].contiguous() if Cin == 1 else x)
    tm = _time_major(case)
    want, packed = _inference_conv(xd, w, b, case, pad, clamp, tm)
    got = train_ops.conv1d_forward(xd, _dev(w), _dev(b), stride, pad, "swish", clamp, tm)
    assert got.dtype == torch.float16 and got.shape == want.shape and torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert bool(torch.isfinite(got).all()) and int(torch.count_nonzero(got)) > 0
    if packed is not None:          # the workspace begins with the device packer's output
        lib = _lib.lib()
        nbytes = lib.bh_conv1d_train_workspace(N, Lin, Cin, Cout, K, stride, pad)
        ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
        lo, hi = clamp if clamp else (-INF, INF)
        os_n, os_t = (Cout, N * Cout) if tm else (want.shape[1] * Cout, Cout)
        wd, bd = _dev(w), _dev(b)
        _lib.check(lib.bh_conv1d_train_forward(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), N, Lin, Cin, Cout, K, stride, pad, 1, lo, hi, os_n,
                                               os_t, _lib.ptr(got), _lib.ptr(ws), nbytes, _lib.stream_ptr()), "bh_conv1d_train_forward")
        torch.cuda.synchronize()
        assert np.array_equal(ws[:packed.size * 2].cpu().numpy().view(np.uint16), packed)


@pytest.mark.parametrize("case", tl.LINEAR_CASES, ids=lambda c: "x".join(str(v) for v in c[:4]))
def test_linear_forward_has_the_bytes_of_bh_linear_with_the_engine_remap(case):
    T, N, K, Cc, act, scale, clamp, bias = case
    x, w, b, dy = tl.linear_inputs(case)
    xd = _dev(x)
    got = train_ops.linear_forward(xd, _dev(w), _dev(b), act, scale, clamp, True)
    plain = train_ops.linear_forward(xd, _dev(w), _dev(b), act, scale, clamp, False)
    want = torch.full((N, T, Cc), -7.0, dtype=torch.float16, device=DEV)
    lo, hi = clamp if clamp else (-INF, INF)
    w16, br = _dev(w.half()), _dev(None if b is None else b.half().float())
    _lib.check(_lib.lib().bh_linear(_lib.ptr(xd), _lib.ptr(w16), _lib.ptr(br), _lib.ptr(want),
                                    T * N, Cc, K, K, K, Cc, _lib.BH_ACT[act], 1.0 if scale is None else scale, lo, hi, 0, N, 1, T, N,
                                    _lib.stream_ptr()), "bh_linear")
    torch.cuda.synchronize()
    assert got.shape == (N, T, Cc) and torch.equal(got.view(torch.int16), want.view(torch.int16))
    assert torch.equal(plain.permute(1, 0, 2), got) and int(torch.count_nonzero(got)) > 0


# ---- backward against the yardstick -------------------------------------------------------------------------------------------------------
def _judge(label, got, exact, yard):
    failed = []
    for name in ("dx", "dw", "db"):
        if exact[name] is None:
            continue
        dk, dy = tl.dist(got[name], exact[name]), tl.dist(yard[name], exact[name])
        print("backward %s %-2s: dist(kernel) = %.3e  dist(yardstick) = %.3e  ratio = %.3f" % (label, name, dk, dy, dk / dy if dy > 0 else INF))
        if not dk <= tl.MARGIN * dy:
            failed.append((name, dk, dy))
    assert not failed, failed


@pytest.mark.parametrize("variant", CONV_VARIANTS, ids=_conv_id)
def test_convolution_backward_within_twice_the_yardstick(variant):
    case, clamp, scale = variant
    x, w, b, dy, pad = tl.conv_inputs(case, scale)
    y, dx, dw, db = _conv_run(case, clamp, scale)
    assert dx.dtype == torch.float16 and dw.dtype == torch.float32 and db.dtype == torch.float32
    m = tl.mask_of(y, clamp)                    # the device's own mask
    if clamp and scale == 4.0:                  # (at scale 1 the small cases have no output beyond a bound)
        assert 0 < int(m.sum()) < m.numel()
    _judge("conv " + _conv_id(variant), {"dx": dx, "dw": dw, "db": db}, tl.conv_exact(x, w, b, m, dy, case[4], pad, "swish"),
           tl.conv_yardstick(x, w, b, m, dy, case[4], pad, "swish"))


@functools.lru_cache(maxsize=None)
def _linear_run(case, batch_major):
    T, N, K, Cc, act, scale, clamp, bias = case
    x, w, b, dy = tl.linear_inputs(case)
    xd, wd, bd = _dev(x), _dev(w), _dev(b)
    y = train_ops.linear_forward(xd, wd, bd, act, scale, clamp, batch_major)
    dyd = _dev(dy).permute(1, 0, 2).contiguous() if batch_major else _dev(dy)
    dx, dw, db = train_ops.linear_backward(xd, wd, y, dyd, act, scale, clamp, batch_major, need_db=bias)
    torch.cuda.synchronize()
    return (y.permute(1, 0, 2) if batch_major else y).cpu(), dx.cpu(), dw.cpu(), None if db is None else db.cpu()


@pytest.mark.parametrize("batch_major", [True, False], ids=["ntc", "tnc"])
@pytest.mark.parametrize("case", tl.LINEAR_CASES, ids=lambda c: "x".join(str(v) for v in c[:4]))
def test_linear_backward_within_twice_the_yardstick(case, batch_major):
    T, N, K, Cc, act, scale, clamp, bias = case
    x, w, b, dy = tl.linear_inputs(case)
    y, dx, dw, db = _linear_run(case, batch_major)
    assert dx.dtype == torch.float16 and dw.dtype == torch.float32 and (db is None) == (not bias)
    m = tl.mask_of(y, clamp)
    if clamp:
        assert 0 < int(m.sum()) < m.numel()
    _judge("linear %s %s" % (case[:4], "ntc" if batch_major else "tnc"), {"dx": dx, "dw": dw, "db": db},
           tl.linear_exact(x, w, b, m, dy, act, scale), tl.linear_yardstick(x, w, b, m, dy, act, scale))
    if batch_major:                  # the layout of Y changes no byte of the gradients
        other = _linear_run(case, False)
        assert torch.equal(dx, other[1]) and torch.equal(dw, other[2])


def test_autograd_of_linear_gives_the_bytes_of_linear_backward():
    case = tl.LINEAR_CASES[1]
    T, N, K, Cc, act, scale, clamp, bias = case
    x, w, b, dy = tl.linear_inputs(case)
    xd, wd, bd = _dev(x).float().requires_grad_(), _dev(w).requires_grad_(), _dev(b).requires_grad_()
    y = train_ops.linear(xd, wd, bd, act, scale, clamp, True)
    y.backward(_dev(dy).permute(1, 0, 2).contiguous())
    _, dx, dw, db = _linear_run(case, True)
    assert xd.grad.dtype == torch.float32 and torch.equal(xd.grad.cpu(), dx.float()) and torch.equal(wd.grad.cpu(), dw) and torch.equal(bd.grad.cpu(), db)
    frozen = _dev(w)
    y = train_ops.linear(_dev(x).requires_grad_(), frozen, None, act, scale, clamp, False)
    y.backward(_dev(dy))
    assert frozen.grad is None


# ---- exact checks -------------------------------------------------------------------------------------------------------------------------
def test_inputs_no_window_reads_have_a_zero_gradient():
    """K = 19, stride 6, padding 1, Lin = 100: (Lin + 2 p - K) mod stride = 5, the 14 windows end at input 95, inputs 96..99 are read by none."""
    g = torch.Generator().manual_seed(5)
    x, w, b = _dev(torch.randn(2, 100, 16, generator=g).half()), _dev(torch.randn(32, 16, 19, generator=g) / 17), _dev(torch.randn(32, generator=g) * 0.1)
    y = train_ops.conv1d_forward(x, w, b, 6, 1, "swish")
    assert y.shape == (2, 14, 32)
    dx, dw, db = train_ops.conv1d_backward(x, w, b, y, torch.ones_like(y), 6, 1, "swish")
    assert int(torch.count_nonzero(dx[:, 96:])) == 0 and int(torch.count_nonzero(dx[:, 95])) > 0 and int(torch.count_nonzero(dx[:, 0])) > 0


def test_a_zero_upstream_gradient_gives_zero_gradients():
    case = tl.CONV_CASES[4]
    x, w, b, dy, pad = tl.conv_inputs(case)
    x, w, b = _dev(x), _dev(w), _dev(b)
    y = train_ops.conv1d_forward(x, w, b, case[4], pad, "swish", tl.CLAMP, True)
    for g in train_ops.conv1d_backward(x, w, b, y, torch.zeros_like(y), case[4], pad, "swish", tl.CLAMP, True):
        assert int(torch.count_nonzero(g)) == 0
    lc = tl.LINEAR_CASES[0]
    X, W, B, dY = (_dev(t) for t in tl.linear_inputs(lc))
    Y = train_ops.linear_forward(X, W, B, "tanh", 5.0, None, True)
    for g in train_ops.linear_backward(X, W, Y, torch.zeros_like(Y), "tanh", 5.0, None, True):
        assert int(torch.count_nonzero(g)) == 0


def test_outputs_on_a_clamp_bound_have_a_zero_gradient():
    """A bias of +-100 puts every output of a channel ON a bound: with dy = 1 everywhere its bias and weight gradients are exactly zero
    (an inclusive mask would give sums of act'), the other channels' are not."""
    case = tl.CONV_CASES[3]
    x, w, b, dy, pad = tl.conv_inputs(case)
    b = b.clone()
    b[:8] = 100.0
    x, w, b = _dev(x), _dev(w), _dev(b)
    y = train_ops.conv1d_forward(x, w, b, 1, pad, "swish", tl.CLAMP)
    assert bool((y[:, :, :8] == tl.CLAMP[1]).all()) and not bool((y[:, :, 8:] == tl.CLAMP[1]).all())
    dx, dw, db = train_ops.conv1d_backward(x, w, b, y, torch.ones_like(y), 1, pad, "swish", tl.CLAMP)
    assert int(torch.count_nonzero(db[:8])) == 0 and int(torch.count_nonzero(dw[:8])) == 0
    assert int(torch.count_nonzero(db[8:])) == 8 and int(torch.count_nonzero(dx)) > 0
    lc = tl.LINEAR_CASES[3]
    X, W, _, dY = (_dev(t) for t in tl.linear_inputs(lc))
    B = torch.zeros(256, device=DEV)
    B[:8], B[8:16] = 100.0, -100.0
    Y = train_ops.linear_forward(X, W, B, None, None, (-5.0, 5.0), True)
    assert bool((Y[:, :, :8] == 5.0).all()) and bool((Y[:, :, 8:16] == -5.0).all())
    dX, dW, dB = train_ops.linear_backward(X, W, Y, torch.ones_like(Y), None, None, (-5.0, 5.0), True)
    assert int(torch.count_nonzero(dB[:16])) == 0 and int(torch.count_nonzero(dW[:16])) == 0 and int(torch.count_nonzero(dB[16:])) > 0


GUARD = 4096


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


def _raw_conv(case, clamp, tm, x, w, b, dy, pad, want_dx=True, want_db=True, override=()):
    """Both entry points on guarded buffers of this test's own -> (dict of _Guarded, rc of the forward, rc of the backward)."""
    N, Cin, Cout, K, stride, Lin = case
    lib = _lib.lib()
    Lout = tl.conv_out_len(Lin, K, stride, pad)
    nbytes = lib.bh_conv1d_train_workspace(N, Lin, Cin, Cout, K, stride, pad)
    assert nbytes > 0
    o = {"y": _Guarded((Lout, N, Cout) if tm else (N, Lout, Cout), torch.float16), "dx": _Guarded(tuple(x.shape), torch.float16),
         "dw": _Guarded((Cout, Cin, K), torch.float32), "db": _Guarded((Cout,), torch.float32), "ws": _Guarded((nbytes,), torch.uint8)}
    lo, hi = clamp if clamp else (-INF, INF)
    os_n, os_t = (Cout, N * Cout) if tm else (Lout * Cout, Cout)
    a = dict(N=N, Lin=Lin, Cin=Cin, Cout=Cout, K=K, stride=stride, pad=pad, act=1)
    a.update(dict(override))
    s = _lib.stream_ptr()
    rf = lib.bh_conv1d_train_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), a["N"], a["Lin"], a["Cin"], a["Cout"], a["K"], a["stride"], a["pad"],
                                     a["act"], lo, hi, os_n, os_t, _lib.ptr(o["y"].t), _lib.ptr(o["ws"].t), nbytes, s)
    ysrc = o["y"].t if rf == 0 else dy
    rb = lib.bh_conv1d_train_backward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(ysrc), _lib.ptr(dy), a["N"], a["Lin"], a["Cin"], a["Cout"],
                                      a["K"], a["stride"], a["pad"], a["act"], lo, hi, os_n, os_t, _lib.ptr(o["dx"].t) if want_dx else None,
                                      _lib.ptr(o["dw"].t), _lib.ptr(o["db"].t) if want_db else None, _lib.ptr(o["ws"].t), nbytes, s)
    torch.cuda.synchronize()
    return o, rf, rb


def _conv_args(case, tm, scale=1.0):
    x, w, b, dy, pad = tl.conv_inputs(case, scale)
    x = x[:, :, 0].contiguous() if case[1] == 1 else x
    return _dev(x), _dev(w), _dev(b), _dev(dy.permute(1, 0, 2).contiguous() if tm else dy), pad


@pytest.mark.parametrize("case", [tl.CONV_CASES[0], tl.CONV_CASES[3], tl.CONV_CASES[4], tl.CONV_CASES[7]], ids=lambda c: "x".join(str(v) for v in c))
def test_convolution_calls_give_equal_bytes_guards_stay_and_null_outputs_are_honoured(case):
    tm = _time_major(case)
    x, w, b, dy, pad = _conv_args(case, tm)
    (a, rf, rb), (c, _, _) = _raw_conv(case, tl.CLAMP, tm, x, w, b, dy, pad), _raw_conv(case, tl.CLAMP, tm, x, w, b, dy, pad)
    assert rf == 0 and rb == 0, _lib.last_error()
    for name in a:
        assert a[name].guards_intact() and c[name].guards_intact(), name
        if name != "ws":                                                     # (the workspace has alignment gaps nobody writes)
            assert torch.equal(a[name].t.view(torch.uint8), c[name].t.view(torch.uint8)), name
            assert bool(torch.isfinite(a[name].t).all()), name
    # ... and they are the bytes the public wrappers return
    y = train_ops.conv1d_forward(x, w, b, case[4], pad, "swish", tl.CLAMP, tm)
    dx, dw, db = train_ops.conv1d_backward(x, w, b, y, dy, case[4], pad, "swish", tl.CLAMP, tm)
    for name, t in (("y", y), ("dx", dx), ("dw", dw), ("db", db)):
        assert torch.equal(a[name].t, t), name
    n, rf, rb = _raw_conv(case, tl.CLAMP, tm, x, w, b, dy, pad, want_dx=False, want_db=False)
    assert rf == 0 and rb == 0 and n["dx"].payload_untouched() and n["db"].payload_untouched() and torch.equal(n["dw"].t, a["dw"].t)


@pytest.mark.parametrize("override,text", [(dict(Cin=12), "Cin must be"), (dict(Cout=98), "Cout must be"), (dict(K=33), "K must be"), (dict(stride=9), "stride must be"),
                                           (dict(pad=19), "pad must be"), (dict(act=7), "unknown activation"), (dict(N=0), "must be positive")],
                         ids=lambda v: "_".join("%s%s" % kv for kv in v.items()) if isinstance(v, dict) else None)
def test_convolution_refusals_launch_nothing(override, text):
    case = tl.CONV_CASES[4]
    x, w, b, dy, pad = _conv_args(case, True)
    o, rf, rb = _raw_conv(case, tl.CLAMP, True, x, w, b, dy, pad, override=override)
    assert rf != 0 and rb != 0 and text in _lib.last_error()
    for name in o:
        assert o[name].payload_untouched(), name


def _raw_linear(case, bm, x, w, b, dy, want_dx=True, want_db=True, **override):
    T, N, K, Cc, act, scale, clamp, bias = case
    lib = _lib.lib()
    nbytes = lib.bh_linear_train_workspace(T, N, K, Cc)
    assert nbytes > 0
    o = {"y": _Guarded((N, T, Cc) if bm else (T, N, Cc), torch.float16), "dx": _Guarded((T, N, K), torch.float16), "dw": _Guarded((Cc, K), torch.float32),
         "db": _Guarded((Cc,), torch.float32), "ws": _Guarded((nbytes,), torch.uint8)}
    lo, hi = clamp if clamp else (-INF, INF)
    a = dict(T=T, N=N, K=K, C=Cc, act=_lib.BH_ACT[act], scale=1.0 if scale is None else scale)
    a.update(override)
    s = _lib.stream_ptr()
    rf = lib.bh_linear_train_forward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), a["T"], a["N"], a["K"], a["C"], a["act"], a["scale"], lo, hi, int(bm),
                                     _lib.ptr(o["y"].t), _lib.ptr(o["ws"].t), nbytes, s)
    ysrc = o["y"].t if rf == 0 else dy
    rb = lib.bh_linear_train_backward(_lib.ptr(x), _lib.ptr(w), _lib.ptr(ysrc), _lib.ptr(dy), a["T"], a["N"], a["K"], a["C"], a["act"], a["scale"], lo,
                                      hi, int(bm), _lib.ptr(o["dx"].t) if want_dx else None, _lib.ptr(o["dw"].t),
                                      _lib.ptr(o["db"].t) if want_db else None, _lib.ptr(o["ws"].t), nbytes, s)
    torch.cuda.synchronize()
    return o, rf, rb


@pytest.mark.parametrize("case", [tl.LINEAR_CASES[1], tl.LINEAR_CASES[3], tl.LINEAR_CASES[4]], ids=lambda c: "x".join(str(v) for v in c[:4]))
def test_linear_calls_give_equal_bytes_guards_stay_and_null_outputs_are_honoured(case):
    T, N, K, Cc, act, scale, clamp, bias = case
    x, w, b, dy = (_dev(t) for t in tl.linear_inputs(case))
    dy = dy.permute(1, 0, 2).contiguous()
    (a, rf, rb), (c, _, _) = _raw_linear(case, True, x, w, b, dy), _raw_linear(case, True, x, w, b, dy)
    assert rf == 0 and rb == 0, _lib.last_error()
    for name in a:
        assert a[name].guards_intact() and c[name].guards_intact(), name
        if name != "ws":
            assert torch.equal(a[name].t.view(torch.uint8), c[name].t.view(torch.uint8)), name
            assert bool(torch.isfinite(a[name].t).all()), name
    y = train_ops.linear_forward(x, w, b, act, scale, clamp, True)
    dx, dw, db = train_ops.linear_backward(x, w, y, dy, act, scale, clamp, True)
    for name, t in (("y", y), ("dx", dx), ("dw", dw), ("db", db)):
        assert torch.equal(a[name].t, t), name
    n, rf, rb = _raw_linear(case, True, x, w, b, dy, want_dx=False, want_db=False)
    assert rf == 0 and rb == 0 and n["dx"].payload_untouched() and n["db"].payload_untouched() and torch.equal(n["dw"].t, a["dw"].t)


@pytest.mark.parametrize("override,text", [(dict(K=100), "K must be"), (dict(C=1020), "C must be"), (dict(act=1), "is not supported"), (dict(scale=0.0), "scale must be"),
                                           (dict(T=0), "must be positive")],
                         ids=lambda v: "_".join("%s%s" % kv for kv in v.items()) if isinstance(v, dict) else None)
def test_linear_refusals_launch_nothing(override, text):
    case = tl.LINEAR_CASES[0]
    x, w, b, dy = (_dev(t) for t in tl.linear_inputs(case))
    o, rf, rb = _raw_linear(case, False, x, w, b, dy, **override)
    assert rf != 0 and rb != 0 and text in _lib.last_error()
    for name in o:
        assert o[name].payload_untouched(), name


def _conv_dx(x, w, b, dy, case, pad, tm):
    y = train_ops.conv1d_forward(x, w, b, case[4], pad, "swish", tl.CLAMP, tm)
    return train_ops.conv1d_backward(x, w, b, y, dy, case[4], pad, "swish", tl.CLAMP, tm)


@pytest.mark.parametrize("tm", [False, True], ids=["ntc", "tnc"])
def test_a_chunk_has_the_same_gradient_in_a_batch_of_3_as_in_a_batch_of_19(tm):
    case = (19, 16, 96, 19, 5, 403)
    x, w, b, dy, pad = tl.conv_inputs(case)
    x, w, b, dy = _dev(x), _dev(w), _dev(b), _dev(dy)
    lay = (lambda t: t.permute(1, 0, 2).contiguous()) if tm else (lambda t: t)
    big = _conv_dx(x, w, b, lay(dy), case, pad, tm)[0]
    small = _conv_dx(x[:3].contiguous(), w, b, lay(dy[:3].contiguous()), (3,) + case[1:], pad, tm)[0]
    assert torch.equal(big[:3], small) and int(torch.count_nonzero(small)) > 0
    lc = (20, 19, 96, 1024, "tanh", 5.0, None, True)
    X, W, B, dY = (_dev(t) for t in tl.linear_inputs(lc))
    Y = train_ops.linear_forward(X, W, B, "tanh", 5.0, None, tm)
    dX = train_ops.linear_backward(X, W, Y, lay(dY), "tanh", 5.0, None, tm)[0]
    Xs, dYs = X[:, :3].contiguous(), dY[:, :3].contiguous()
    Ys = train_ops.linear_forward(Xs, W, B, "tanh", 5.0, None, tm)
    assert torch.equal(Ys, Y[:3] if tm else Y[:, :3])
    assert torch.equal(train_ops.linear_backward(Xs, W, Ys, lay(dYs), "tanh", 5.0, None, tm)[0], dX[:, :3])


def test_a_non_finite_upstream_gradient_stays_in_its_chunk():
    case = tl.CONV_CASES[4]
    x, w, b, dy, pad = _conv_args(case, True)
    clean = _conv_dx(x, w, b, dy, case, pad, True)
    bad = dy.clone()
    bad[7, 1, :] = INF
    dx, dw, db = _conv_dx(x, w, b, bad, case, pad, True)
    assert torch.equal(dx[[0, 2]], clean[0][[0, 2]]) and bool(torch.isfinite(clean[0]).all()) and not bool(torch.isfinite(dx[1]).all())
    assert not bool(torch.isfinite(dw).all()) and not bool(torch.isfinite(db).all())
    lc = tl.LINEAR_CASES[0]
    X, W, B, dY = (_dev(t) for t in tl.linear_inputs(lc))
    Y = train_ops.linear_forward(X, W, B, "tanh", 5.0, None, False)
    clean = train_ops.linear_backward(X, W, Y, dY, "tanh", 5.0, None, False)[0]
    bad = dY.clone()
    bad[4, 1, :] = INF
    dX = train_ops.linear_backward(X, W, Y, bad, "tanh", 5.0, None, False)[0]
    assert torch.equal(dX[:, [0, 2]], clean[:, [0, 2]]) and not bool(torch.isfinite(dX[:, 1]).all())


def test_linear_backward_past_2_to_the_31_elements():
    """M C = (2^19 + 16) x 4096 > 2^31 elements of dY and dZ, K = 32; every block of 16 rows is a copy of the first. dX of every block
    must have the bytes of the 16-row case. dW is M / 16 times the 16-row case's up to the fp32 sums: the rows are split into 16 blocks
    of 32800 rows, a workgroup adds the 32800 / 32 = 1025 MFMA results of an element in sequence (each the same number, so the running
    sum grows linearly and every addition is within 2^-24 relative of at most the final sum), then the 16 partial sums are added in
    order: (1025 + 16) additions, doubled for the rounding inside an MFMA and of the 16-row case itself: 2 x 1041 x 2^-24 = 1.3e-4.
    db: some 1024 partial sums of 513 rows each, then as many additions: 2 x 1537 x 2^-24 = 1.9e-4."""
    K, Cc, N = 32, 4096, 16
    T = (2 ** 19 + 16) // N
    g = torch.Generator().manual_seed(11)
    x16, dy16 = _dev(torch.randn(1, N, K, generator=g).half()), _dev(torch.randn(1, N, Cc, generator=g).half())
    w = _dev(torch.randn(Cc, K, generator=g) / 6)
    dx16, dw16, db16 = train_ops.linear_backward(x16, w, dy16, dy16, None, None, None, False)
    x, dy = x16.expand(T, N, K).contiguous(), dy16.expand(T, N, Cc).contiguous()
    assert dy.numel() > 2 ** 31
    dx, dw, db = train_ops.linear_backward(x, w, dy, dy, None, None, None, False)       # (no activation, no clamp: Y is not read)
    torch.cuda.synchronize()
    assert torch.equal(dx, dx16.expand(T, N, K)) and int(torch.count_nonzero(dx[-1])) > 0
    for name, big, small, adds in (("dW", dw, dw16, 1025 + 16), ("db", db, db16, 513 + 1024)):
        d, bound = tl.dist(big, small.double() * T), 2 * adds * 2.0 ** -24
        print("large %s: distance from %d x the 16-row case = %.3e (bound %.3e)" % (name, T, d, bound))
        assert d <= bound, name

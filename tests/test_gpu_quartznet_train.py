"""What training a QuartzNet CTC model adds, on the device (-m gpu): bh_dwconv1d_train_backward, bh_residual_act_train_forward / _backward,
bh_ctc_head_train_backward and bonito_amd.train_ops.depthwise_conv1d / residual_act / ctc_head.

exact = fp64 torch under autograd, yardstick = the same layer in fp16 on the CPU (tests/quartznet_train_ref.py, pinned by
tests/test_quartznet_train_ref_cpu.py). With dist(a) = max|a - exact| / max|exact| every output must satisfy
dist(kernel) <= 2 dist(yardstick); every case prints its figures first. The dropout mask of the references is the restatement's keep
function in integers, so y and da pin the device's mask to it bit for bit: one differing element is an error of the size of the value.

The rest is exact: the forward bytes are those of bh_dwconv1d / bh_ctc_head, equal bytes from call to call, untouched guard bytes around
every output and the workspace, null outputs, refused calls that launch nothing, 64-bit indexing where N L C passes 2^31."""
import functools

import pytest
import torch

import quartznet_train_ref as ref
from bonito_amd import _lib, train_ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 512
SEED, STREAM = 0x1234567890ABCDEF, 3
# (N, L, C, K, pad)
DW_SHAPES = [(1, 1, 8, 1, 0), (1, 5, 8, 9, 4), (2, 64, 64, 5, 2), (3, 65, 72, 33, 16), (2, 130, 8, 123, 61), (1, 200, 136, 31, 15),
             (2, 70, 16, 4, 2), (2, 9, 8, 3, 0)]
HEAD_SHAPES = [(M, Fe, classes) for M in (1, 255, 257, 600) for Fe in (8, 40, 384) for classes in (2, 5, 8)]


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


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _held(got, exact, yard, names, label):
    bad = ref.within(got, exact, yard, names, label)
    assert not bad, (label, bad)


# ---- depthwise convolution -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dw(shape):
    case = ref.dw_case(*shape)
    return case, {k: case[k].to(DEV) for k in ("x", "w", "dy")}, ref.dw_exact(case), ref.dw_yardstick(case)


def _dw_raw(shape, dx=True, dw=True):
    N, L, C, K, pad = shape
    _, dev, _, _ = _dw(shape)
    lib, s = _lib.lib(), _lib.stream_ptr()
    nbytes = lib.bh_dwconv1d_train_workspace(N, L, C, K, pad)
    assert nbytes >= ref.dw_blocks(N, L, C, K, pad)[2] * C * K * 4
    o = {"dx": _Guarded((N, L, C), torch.float16), "dw": _Guarded((C, 1, K), torch.float32), "ws": _Guarded((nbytes,), torch.uint8)}
    _lib.check(lib.bh_dwconv1d_train_backward(_lib.ptr(dev["x"]), _lib.ptr(dev["w"]), _lib.ptr(dev["dy"]), N, L, C, K, pad,
                                              _lib.ptr(o["dx"].t) if dx else None, _lib.ptr(o["dw"].t) if dw else None, _lib.ptr(o["ws"].t),
                                              nbytes, s), "bh_dwconv1d_train_backward")
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("shape", DW_SHAPES)
def test_depthwise_backward_against_fp64(shape):
    N, L, C, K, pad = shape
    case, dev, exact, yard = _dw(shape)
    y = train_ops.depthwise_conv1d_forward(dev["x"], dev["w"], pad)
    want = torch.empty_like(y)
    _lib.check(_lib.lib().bh_dwconv1d(_lib.ptr(dev["x"]), _lib.ptr(dev["w"]), _lib.ptr(want), N, L, C, K, 1, pad, _lib.stream_ptr()), "bh_dwconv1d")
    assert _same_bytes(y, want)
    o = _dw_raw(shape)
    assert all(o[k].guards_intact() for k in o)
    got = {"y": y.cpu(), "dx": o["dx"].t.cpu(), "dw": o["dw"].t.cpu()}
    _held(got, exact, yard, ("y", "dx", "dw"), "dwconv %s" % (shape,))
    again = _dw_raw(shape)
    assert _same_bytes(o["dx"].t, again["dx"].t) and _same_bytes(o["dw"].t, again["dw"].t)
    dx, dw = train_ops.depthwise_conv1d_backward(dev["x"], dev["w"], dev["dy"], pad)
    assert _same_bytes(dx, o["dx"].t) and _same_bytes(dw, o["dw"].t)


def test_depthwise_null_outputs_and_refusals():
    shape = (3, 65, 72, 33, 16)
    N, L, C, K, pad = shape
    full = _dw_raw(shape)
    only_dx, only_dw = _dw_raw(shape, dw=False), _dw_raw(shape, dx=False)
    assert only_dx["dw"].payload_untouched() and only_dw["dx"].payload_untouched()
    assert _same_bytes(only_dx["dx"].t, full["dx"].t) and _same_bytes(only_dw["dw"].t, full["dw"].t)
    assert all(o[k].guards_intact() for o in (only_dx, only_dw) for k in o)
    _, dev, _, _ = _dw(shape)
    lib, s = _lib.lib(), _lib.stream_ptr()
    nbytes = lib.bh_dwconv1d_train_workspace(*shape)
    o = {"dx": _Guarded((N, L, C), torch.float16), "dw": _Guarded((C, 1, K), torch.float32), "ws": _Guarded((nbytes,), torch.uint8)}

    def call(N=N, L=L, C=C, K=K, pad=pad, nbytes=nbytes, x=dev["x"]):
        return lib.bh_dwconv1d_train_backward(_lib.ptr(x), _lib.ptr(dev["w"]), _lib.ptr(dev["dy"]), N, L, C, K, pad, _lib.ptr(o["dx"].t),
                                              _lib.ptr(o["dw"].t), _lib.ptr(o["ws"].t), nbytes, s)

    for kw, text in [(dict(C=68), "multiple of 8"), (dict(K=128), "1..127"), (dict(K=0), "1..127"), (dict(pad=33), "0..K-1"),
                     (dict(pad=-1), "0..K-1"), (dict(L=10, pad=0), "shorter than one window"), (dict(N=0), "positive"),
                     (dict(nbytes=nbytes - 1), "workspace of"), (dict(x=None), "null pointer"),
                     (dict(x=dev["x"].view(-1)[4:]), "16-byte aligned")]:
        assert call(**kw) != 0 and text in _lib.last_error(), (kw, _lib.last_error())
    torch.cuda.synchronize()
    assert all(o[k].payload_untouched() for k in o)
    assert call() == 0


def test_depthwise_autograd_layer():
    shape = (3, 65, 72, 33, 16)
    case, dev, exact, yard = _dw(shape)
    x, w = dev["x"].float().requires_grad_(), dev["w"].clone().requires_grad_()
    y = train_ops.depthwise_conv1d(x, w, 16)
    y.backward(dev["dy"])
    o = _dw_raw(shape)
    assert x.grad.dtype == torch.float32 and _same_bytes(x.grad.half(), o["dx"].t) and _same_bytes(w.grad, o["dw"].t)
    w2 = dev["w"].clone().requires_grad_()
    train_ops.depthwise_conv1d(dev["x"], w2, 16).backward(dev["dy"])           # no gradient asked for x
    assert _same_bytes(w2.grad, o["dw"].t)


def test_depthwise_past_2_31_elements():
    """N L C = 2 * 16777280 * 64 > 2^31: x and dy are zero but for K-row-separated slices at both ends of the buffers, so that dx on the
    slices and the whole of dw have the references of the slices."""
    N, L, C, K, pad, S = 2, (1 << 24) + 64, 64, 5, 2, 192
    assert N * L * C > 1 << 31
    head, tail = ref.dw_case(1, S, C, K, pad, seed=1), ref.dw_case(1, S, C, K, pad, seed=2)
    w = head["w"]
    tail["w"] = w
    x, dy = torch.zeros((N, L, C), dtype=torch.float16, device=DEV), torch.zeros((N, L, C), dtype=torch.float16, device=DEV)
    x[0, :S], dy[0, :S], x[1, L - S:], dy[1, L - S:] = head["x"][0].to(DEV), head["dy"][0].to(DEV), tail["x"][0].to(DEV), tail["dy"][0].to(DEV)
    dx, dw = train_ops.depthwise_conv1d_backward(x, w.to(DEV), dy, pad)
    y = train_ops.depthwise_conv1d_forward(x, w.to(DEV), pad)
    torch.cuda.synchronize()
    for case, n, sl in ((head, 0, slice(0, S)), (tail, 1, slice(L - S, L))):
        exact, yard = ref.dw_exact(case), ref.dw_yardstick(case)
        _held({"y": y[n, sl][None].cpu(), "dx": dx[n, sl][None].cpu()}, exact, yard, ("y", "dx"), "dwconv 2^31 item %d" % n)
    assert int(torch.count_nonzero(dx[0, S + K:])) == 0 and int(torch.count_nonzero(dx[1, :L - S - K])) == 0
    exact = ref.dw_exact(head)["dw"] + ref.dw_exact(tail)["dw"]
    yard = ref.dw_yardstick(head)["dw"].double() + ref.dw_yardstick(tail)["dw"].double()
    _held({"dw": dw.cpu()}, {"dw": exact}, {"dw": yard}, ("dw",), "dwconv 2^31")


# ---- CTC head -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _head(shape):
    case = ref.head_case(*shape)
    return case, {k: v.to(DEV) for k, v in case.items()}, ref.head_exact(case), ref.head_yardstick(case)


def _head_raw(shape, dx=True, dw=True, db=True):
    M, Fe, classes = shape
    _, dev, _, _ = _head(shape)
    lib, s = _lib.lib(), _lib.stream_ptr()
    nbytes = lib.bh_ctc_head_train_workspace(M, Fe, classes)
    assert nbytes >= M * 8 * 4
    o = {"dx": _Guarded((M, Fe), torch.float16), "dw": _Guarded((classes, Fe), torch.float32), "db": _Guarded((classes,), torch.float32),
         "ws": _Guarded((nbytes,), torch.uint8)}
    _lib.check(lib.bh_ctc_head_train_backward(_lib.ptr(dev["x"]), _lib.ptr(dev["w"]), _lib.ptr(dev["b"]), _lib.ptr(dev["dlp"]), M, Fe, classes,
                                              _lib.ptr(o["dx"].t) if dx else None, _lib.ptr(o["dw"].t) if dw else None,
                                              _lib.ptr(o["db"].t) if db else None, _lib.ptr(o["ws"].t), nbytes, s), "bh_ctc_head_train_backward")
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("shape", HEAD_SHAPES)
def test_head_backward_against_fp64(shape):
    M, Fe, classes = shape
    case, dev, exact, yard = _head(shape)
    lp = train_ops.ctc_head_forward(dev["x"][None], dev["w"][:, :, None], dev["b"])[0]
    want = torch.empty_like(lp)
    _lib.check(_lib.lib().bh_ctc_head(_lib.ptr(dev["x"]), _lib.ptr(dev["w"]), _lib.ptr(dev["b"]), _lib.ptr(want), M, Fe, classes, _lib.stream_ptr()),
               "bh_ctc_head")
    assert _same_bytes(lp, want)
    o = _head_raw(shape)
    assert all(o[k].guards_intact() for k in o)
    got = {"lp": lp.cpu(), **{k: o[k].t.cpu() for k in ("dx", "dw", "db")}}
    _held(got, exact, yard, ("lp", "dx", "dw", "db"), "ctc head %s" % (shape,))
    again = _head_raw(shape)
    assert all(_same_bytes(o[k].t, again[k].t) for k in ("dx", "dw", "db"))


def test_head_null_outputs_refusals_and_autograd():
    shape = (257, 384, 8)
    M, Fe, classes = shape
    full = _head_raw(shape)
    for absent in ("dx", "dw", "db"):
        o = _head_raw(shape, **{absent: False})
        assert o[absent].payload_untouched() and all(o[k].guards_intact() for k in o)
        assert all(_same_bytes(o[k].t, full[k].t) for k in ("dx", "dw", "db") if k != absent)
    _, dev, _, _ = _head(shape)
    lib, s = _lib.lib(), _lib.stream_ptr()
    nbytes = lib.bh_ctc_head_train_workspace(*shape)
    o = {"dx": _Guarded((M, Fe), torch.float16), "dw": _Guarded((classes, Fe), torch.float32), "db": _Guarded((classes,), torch.float32),
         "ws": _Guarded((nbytes,), torch.uint8)}

    def call(M=M, Fe=Fe, classes=classes, nbytes=nbytes, dlp=dev["dlp"]):
        return lib.bh_ctc_head_train_backward(_lib.ptr(dev["x"]), _lib.ptr(dev["w"]), _lib.ptr(dev["b"]), _lib.ptr(dlp), M, Fe, classes,
                                              _lib.ptr(o["dx"].t), _lib.ptr(o["dw"].t), _lib.ptr(o["db"].t), _lib.ptr(o["ws"].t), nbytes, s)

    for kw, text in [(dict(classes=9), "1..8"), (dict(Fe=380), "multiple of 8"), (dict(Fe=4096), "64 KiB"), (dict(M=0), "positive"),
                     (dict(nbytes=nbytes - 1), "workspace of"), (dict(dlp=None), "null pointer")]:
        assert call(**kw) != 0 and text in _lib.last_error(), (kw, _lib.last_error())
    torch.cuda.synchronize()
    assert all(o[k].payload_untouched() for k in o)
    x = dev["x"].reshape(1, M, Fe).float().requires_grad_()
    w, b = dev["w"][:, :, None].clone().requires_grad_(), dev["b"].clone().requires_grad_()
    train_ops.ctc_head(x, w, b).backward(dev["dlp"][None])
    assert _same_bytes(x.grad.half()[0], full["dx"].t) and _same_bytes(w.grad[:, :, 0], full["dw"].t) and _same_bytes(b.grad, full["db"].t)


# ---- residual add + activation + dropout ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 8), (3 * 65, 72)])
@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.05, 0.5])
def test_residual_act_against_fp64_under_the_integer_mask(shape, with_b, p):
    M, C = shape
    case = ref.res_case(M, C, with_b)
    a, dy = case["a"].to(DEV), case["dy"].to(DEV)
    b = case["b"].to(DEV) if with_b else None
    mask = ref.res_mask(case, p, SEED, STREAM)
    lib, s = _lib.lib(), _lib.stream_ptr()
    thr, inv = train_ops.keep_threshold(p)
    for act in ref.ACTS:
        o = {"y": _Guarded((M, C), torch.float16), "da": _Guarded((M, C), torch.float16)}
        _lib.check(lib.bh_residual_act_train_forward(_lib.ptr(a), _lib.ptr(b), M, C, _lib.BH_ACT[act], thr, inv, SEED, STREAM, _lib.ptr(o["y"].t), s),
                   "bh_residual_act_train_forward")
        _lib.check(lib.bh_residual_act_train_backward(_lib.ptr(a), _lib.ptr(b), _lib.ptr(dy), M, C, _lib.BH_ACT[act], thr, inv, SEED, STREAM,
                                                      _lib.ptr(o["da"].t), s), "bh_residual_act_train_backward")
        torch.cuda.synchronize()
        assert o["y"].guards_intact() and o["da"].guards_intact()
        got = {"y": o["y"].t.cpu(), "da": o["da"].t.cpu()}
        if p > 0 and M > 1:       # the kept set IS the integer function's: a dropped element is an exact zero, a kept swish value is not
            assert torch.equal(got["y"][~mask], torch.zeros_like(got["y"][~mask])) and torch.equal(got["da"][~mask], torch.zeros_like(got["da"][~mask]))
        _held(got, ref.res_exact(case, act, p, mask), ref.res_yardstick(case, act, p, mask), ("y", "da"),
              "residual_act %s b=%s p=%g %s" % (shape, with_b, p, act))
        y = train_ops.residual_act_forward(a, b, act, p, SEED, STREAM)
        assert _same_bytes(y, o["y"].t) and _same_bytes(train_ops.residual_act_backward(a, b, dy, act, p, SEED, STREAM), o["da"].t)
        if p == 0.0:              # the bytes of fp16(act(a + b)): no trace of seed or stream, and for the exactly rounded activations numpy's
            assert _same_bytes(y, train_ops.residual_act_forward(a, b, act, 0.0, SEED + 1, STREAM + 1))
            if act in ("none", "relu"):
                u = case["a"].float() + (case["b"].float() if with_b else 0.0)
                assert torch.equal(got["y"], ref.act_fn(u, act).half())
        else:
            other = train_ops.residual_act_forward(a, b, act, p, SEED, STREAM + 1)
            assert M == 1 or not _same_bytes(y, other)


def test_residual_act_mask_at_p_half_and_autograd():
    """With act none and b absent y = 2 a on the kept elements exactly: the device's kept set against the integer function, bit for bit."""
    M, C = 3 * 65, 72
    case = ref.res_case(M, C, True)
    a, b, dy = (case[k].to(DEV) for k in ("a", "b", "dy"))
    y = train_ops.residual_act_forward(a, None, "none", 0.5, SEED, STREAM).cpu()
    mask = ref.res_mask(case, 0.5, SEED, STREAM)
    assert torch.equal(y, (case["a"].float() * 2.0 * mask).half())
    a32, b16 = a.float().requires_grad_(), b.clone().requires_grad_()
    train_ops.residual_act(a32, b16, "swish", 0.05, SEED, STREAM).backward(dy)
    da = train_ops.residual_act_backward(a, b, dy, "swish", 0.05, SEED, STREAM)
    assert a32.grad.dtype == torch.float32 and _same_bytes(a32.grad.half(), da) and _same_bytes(b16.grad, da)
    lone = a.clone().requires_grad_()
    train_ops.residual_act(lone, None, "tanh", 0.5, SEED, 7).backward(dy)
    assert _same_bytes(lone.grad, train_ops.residual_act_backward(a, None, dy, "tanh", 0.5, SEED, 7))
    lib = _lib.lib()
    out = _Guarded((M, C), torch.float16)
    for kw, text in [(dict(C=12), "multiple of 8"), (dict(act=9), "unknown activation"), (dict(inv=0.5), "inv_keep"), (dict(M=0), "positive")]:
        args = dict(M=M, C=C, act=1, inv=2.0)
        args.update(kw)
        rc = lib.bh_residual_act_train_forward(_lib.ptr(a), None, args["M"], args["C"], args["act"], 1 << 31, args["inv"], SEED, STREAM, _lib.ptr(out.t),
                                               _lib.stream_ptr())
        assert rc != 0 and text in _lib.last_error(), (kw, _lib.last_error())
    torch.cuda.synchronize()
    assert out.payload_untouched()

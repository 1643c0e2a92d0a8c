"""What a transformer encoder layer adds to training, on the device (-m gpu): bh_rmsnorm_train_backward, bh_gated_linear_train_forward /
_backward, bonito_amd.train_ops.rmsnorm_residual / gated_linear and bonito_amd.attn.encoder_layer.

FORWARD. The norm has the bytes of bh_rmsnorm_residual, the gated layer the bytes of bh_linear(gated = 1) on host-interleaved rounded
weights: what the engine computes.

BACKWARD. exact = fp64 torch autograd through the layer restated in torch ops (tests/transformer_train_ref.py, pinned against the
written-out formulas and central differences by tests/test_transformer_train_ref_cpu.py); yardstick = the same restatement run by torch
in fp16 on the CPU. With dist(a) = max|a - exact| / max|exact|, every output must satisfy dist(kernel) <= 2 dist(yardstick): the
project's margin for composed training layers. An fp32 emulation of the design with fp16 storage is inside it and every planted defect
outside (the CPU file). Every case prints its ratios; DESIGN.md section 6 records them.

The rest is exact: equal bytes from call to call, untouched guard bytes, a null da or dx that leaves the other output's bytes alone, dW1
in torch's row order, 64-bit indexing where M * 2F passes 2^31."""
import functools

import pytest
import torch

import transformer_train_ref as ref
from bonito_amd import _lib, attn, train_ops
from bonito_amd.transformer.model import TransformerEncoderLayer

pytestmark = pytest.mark.gpu

DEV = "cuda"
V5_ALPHA = 2.4494897
INF = float("inf")
GUARD = 512


def _dev(case):
    return {k: v.to(DEV) for k, v in case.items()}


def _check(label, names, got, exact, yard):
    failed = []
    for name, g, e, y in zip(names, got, exact, yard):
        dk, dy = ref.dist(g, e), ref.dist(y, e)
        print("%s %-26s: dist(kernel) = %.3e  dist(yardstick) = %.3e  ratio = %.3f" % (label, name, dk, dy, dk / dy if dy > 0 else INF))
        if not dk <= ref.MARGIN * dy:
            failed.append((name, dk, dy))
    assert not failed, failed


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


# ---- norm -------------------------------------------------------------------------------------------------------------------------------------
NORM_D = (8, 64, 512, 520, 1024)         # 520: a second, partly filled vector per lane
NORM_M = (1, 3, 4, 5, 257)               # four rows per workgroup, tails, more than one dw block


@functools.lru_cache(maxsize=None)
def _norm_refs(M, D, alpha, zero_row=None):
    """(case, exact, yardstick), computed once on the CPU and never modified."""
    case = ref.norm_case(M, D, zero_row=zero_row)
    return case, ref.norm_torch(case, alpha), ref.norm_torch(case, alpha, dtype=torch.float16)


def _norm_run(M, D, alpha, zero_row=None):
    case, exact, yard = _norm_refs(M, D, alpha, zero_row)
    c = _dev(case)
    out = train_ops.rmsnorm_residual_forward(c["a"], c["x"], c["w"], alpha)
    da, dx, dw = train_ops.rmsnorm_residual_backward(c["a"], c["x"], c["w"], c["dy"], alpha)
    torch.cuda.synchronize()
    assert out.dtype == da.dtype == dx.dtype == torch.float16 and dw.dtype == torch.float32 and tuple(dw.shape) == (D,)
    want = torch.full_like(out, float("nan"))
    _lib.check(_lib.lib().bh_rmsnorm_residual(_lib.ptr(c["a"]), _lib.ptr(c["x"]), _lib.ptr(c["w"]), _lib.ptr(want), M, D, alpha, ref.EPS,
                                              _lib.stream_ptr()), "bh_rmsnorm_residual")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(want).all()) and _same_bytes(out, want)            # the forward IS the engine's kernel
    _check("norm M=%d D=%d alpha=%g%s" % (M, D, alpha, "" if zero_row is None else " zero row"), ref.NORM_NAMES, (out, da, dx, dw), exact, yard)
    return out, da, dx, dw


@pytest.mark.parametrize("M", NORM_M)
@pytest.mark.parametrize("D", NORM_D)
def test_norm_within_twice_the_yardstick(D, M):
    _norm_run(M, D, V5_ALPHA)


@pytest.mark.parametrize("M,D", ((5, 64), (257, 520)))
def test_norm_with_alpha_one(M, D):
    _norm_run(M, D, 1.0)


def test_norm_with_an_all_zero_row():
    out, da, dx, dw = _norm_run(5, 64, V5_ALPHA, zero_row=2)
    assert int(torch.count_nonzero(out[2])) == 0 and bool(torch.isfinite(da).all()) and int(torch.count_nonzero(da[2])) > 0


def _norm_raw(c, M, D, alpha, da=True, dx=True):
    lib = _lib.lib()
    nbytes = lib.bh_rmsnorm_train_workspace(M, D)
    assert nbytes >= ((M + 63) // 64) * D * 4
    o = {"da": _Guarded((M, D), torch.float16), "dx": _Guarded((M, D), torch.float16), "dw": _Guarded((D,), torch.float32),
         "ws": _Guarded((nbytes,), torch.uint8)}
    _lib.check(lib.bh_rmsnorm_train_backward(_lib.ptr(c["a"]), _lib.ptr(c["x"]), _lib.ptr(c["w"]), _lib.ptr(c["dy"]), M, D, alpha, ref.EPS,
                                             _lib.ptr(o["da"].t) if da else None, _lib.ptr(o["dx"].t) if dx else None, _lib.ptr(o["dw"].t),
                                             _lib.ptr(o["ws"].t), nbytes, _lib.stream_ptr()), "bh_rmsnorm_train_backward")
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("M,D", ((257, 520), (5, 8), (130, 1024)))
def test_norm_equal_bytes_guard_bytes_and_null_outputs(M, D):
    c = _dev(ref.norm_case(M, D))
    first, second = _norm_raw(c, M, D, V5_ALPHA), _norm_raw(c, M, D, V5_ALPHA)
    for o in (first, second):
        for name in o:
            assert o[name].guards_intact(), name
    for name in ("da", "dx", "dw"):
        assert _same_bytes(first[name].t, second[name].t) and bool(torch.isfinite(first[name].t).all()), name
    da, dx, dw = train_ops.rmsnorm_residual_backward(c["a"], c["x"], c["w"], c["dy"], V5_ALPHA)      # ... and they are the wrapper's bytes
    assert _same_bytes(da, first["da"].t) and _same_bytes(dx, first["dx"].t) and _same_bytes(dw, first["dw"].t)
    no_da, no_dx = _norm_raw(c, M, D, V5_ALPHA, da=False), _norm_raw(c, M, D, V5_ALPHA, dx=False)
    assert no_da["da"].payload_untouched() and _same_bytes(no_da["dx"].t, first["dx"].t) and _same_bytes(no_da["dw"].t, first["dw"].t)
    assert no_dx["dx"].payload_untouched() and _same_bytes(no_dx["da"].t, first["da"].t) and _same_bytes(no_dx["dw"].t, first["dw"].t)


def test_norm_refused_calls_leave_the_outputs_untouched():
    M, D = 5, 64
    c = _dev(ref.norm_case(M, D))
    lib, s = _lib.lib(), _lib.stream_ptr()
    o = {"da": _Guarded((M, D), torch.float16), "dw": _Guarded((D,), torch.float32), "ws": _Guarded((4096,), torch.uint8)}

    def call(D=D, ws_bytes=4096):
        return lib.bh_rmsnorm_train_backward(_lib.ptr(c["a"]), _lib.ptr(c["x"]), _lib.ptr(c["w"]), _lib.ptr(c["dy"]), M, D, 1.0, ref.EPS,
                                             _lib.ptr(o["da"].t), None, _lib.ptr(o["dw"].t), _lib.ptr(o["ws"].t), ws_bytes, s)

    assert call(D=60) != 0 and "multiple of 8" in _lib.last_error()
    assert call(ws_bytes=16) != 0 and "workspace of" in _lib.last_error()
    torch.cuda.synchronize()
    for name in o:
        assert o[name].payload_untouched(), name


def test_norm_autograd_hands_on_the_bytes_and_the_dtypes():
    M, D = 37, 128
    c = _dev(ref.norm_case(M, D))
    da, dx, dw = train_ops.rmsnorm_residual_backward(c["a"], c["x"], c["w"], c["dy"], V5_ALPHA)
    a, x, w = c["a"].clone().requires_grad_(), c["x"].float().requires_grad_(), c["w"].clone().requires_grad_()
    out = train_ops.rmsnorm_residual(a, x, w, torch.tensor(V5_ALPHA, device=DEV))
    assert _same_bytes(out.detach(), train_ops.rmsnorm_residual_forward(c["a"], c["x"], c["w"], V5_ALPHA))
    out.backward(c["dy"])
    assert a.grad.dtype == torch.float16 and _same_bytes(a.grad, da)
    assert x.grad.dtype == torch.float32 and torch.equal(x.grad, dx.float())                 # the residual's gradient in its dtype
    assert w.grad.dtype == torch.float32 and _same_bytes(w.grad, dw)


# ---- gated layer --------------------------------------------------------------------------------------------------------------------------------
GATED_SHAPES = ((8, 8, 1), (64, 72, 17), (128, 256, 130), (512, 2048, 33))       # (D, F, M)


@functools.lru_cache(maxsize=None)
def _gated_refs(D, F, M):
    case = ref.gated_case(M, D, F)
    return case, ref.gated_torch(case), ref.gated_torch(case, dtype=torch.float16)


def _engine_fc1(x, w, M, D, F):
    """bh_linear with gated = 1 on the rounded weights, rows interleaved (y_j, gate_j) on the host: the engine's fc1."""
    wi = torch.stack([w[:F], w[F:]], dim=1).reshape(2 * F, D).half().contiguous()
    out = torch.full((M, F), float("nan"), dtype=torch.float16, device=DEV)
    _lib.check(_lib.lib().bh_linear(_lib.ptr(x), _lib.ptr(wi), None, _lib.ptr(out), M, 2 * F, D, D, D, F, 0, 1.0, -INF, INF, 1, 0, 0, 0, 0,
                                    _lib.stream_ptr()), "bh_linear")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("D,F,M", GATED_SHAPES)
def test_gated_layer_forward_bytes_and_backward_within_twice_the_yardstick(D, F, M):
    case, exact, yard = _gated_refs(D, F, M)
    c = _dev(case)
    h = train_ops.gated_linear_forward(c["x"], c["w"])
    dx, dw = train_ops.gated_linear_backward(c["x"], c["w"], c["dh"])
    torch.cuda.synchronize()
    assert h.dtype == dx.dtype == torch.float16 and tuple(h.shape) == (M, F) and dw.dtype == torch.float32 and tuple(dw.shape) == (2 * F, D)
    want = _engine_fc1(c["x"], c["w"], M, D, F)
    assert bool(torch.isfinite(want).all()) and _same_bytes(h, want)
    _check("gated D=%d F=%d M=%d" % (D, F, M), ref.GATED_NAMES, (h, dx, dw), exact, yard)
    # dW1 is in torch's row order: the y rows and the gate rows have visibly different gradients, and the interleaved order is far outside
    e = exact[2]
    assert ref.dist(e[:F], e[F:]) > 0.5
    swapped = torch.stack([dw[:F], dw[F:]], dim=1).reshape(2 * F, D)
    assert ref.dist(swapped, e) > 10 * ref.MARGIN * ref.dist(yard[2], e)


def _gated_raw(c, M, D, F, dx=True):
    lib = _lib.lib()
    nbytes = lib.bh_gated_linear_train_workspace(M, D, F)
    assert nbytes >= M * 2 * F * 2 + 2 * F * D * 2
    o = {"h": _Guarded((M, F), torch.float16), "dx": _Guarded((M, D), torch.float16), "dw": _Guarded((2 * F, D), torch.float32),
         "ws": _Guarded((nbytes,), torch.uint8)}
    _lib.check(lib.bh_gated_linear_train_forward(_lib.ptr(c["x"]), _lib.ptr(c["w"]), M, D, F, _lib.ptr(o["h"].t), _lib.ptr(o["ws"].t), nbytes,
                                                 _lib.stream_ptr()), "bh_gated_linear_train_forward")
    _lib.check(lib.bh_gated_linear_train_backward(_lib.ptr(c["x"]), _lib.ptr(c["w"]), _lib.ptr(c["dh"]), M, D, F, _lib.ptr(o["dx"].t) if dx else None,
                                                  _lib.ptr(o["dw"].t), _lib.ptr(o["ws"].t), nbytes, _lib.stream_ptr()),
               "bh_gated_linear_train_backward")
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("D,F,M", ((64, 72, 17), (128, 256, 1030)))
def test_gated_layer_equal_bytes_guard_bytes_and_a_null_dx(D, F, M):
    c = _dev(ref.gated_case(M, D, F))
    first, second, no_dx = _gated_raw(c, M, D, F), _gated_raw(c, M, D, F), _gated_raw(c, M, D, F, dx=False)
    for o in (first, second, no_dx):
        for name in o:
            assert o[name].guards_intact(), name
    for name in ("h", "dx", "dw"):
        assert _same_bytes(first[name].t, second[name].t) and bool(torch.isfinite(first[name].t).all()), name
    assert no_dx["dx"].payload_untouched() and _same_bytes(no_dx["dw"].t, first["dw"].t)
    dx, dw = train_ops.gated_linear_backward(c["x"], c["w"], c["dh"])
    assert _same_bytes(dx, first["dx"].t) and _same_bytes(dw, first["dw"].t)
    lib = _lib.lib()
    o = first
    assert lib.bh_gated_linear_train_forward(_lib.ptr(c["x"]), _lib.ptr(c["w"]), M, D, F, _lib.ptr(o["h"].t), _lib.ptr(o["ws"].t), 256,
                                             _lib.stream_ptr()) != 0 and "workspace of" in _lib.last_error()
    assert lib.bh_gated_linear_train_backward(_lib.ptr(c["x"]), _lib.ptr(c["w"]), _lib.ptr(c["dh"]), M, D, F + 4, None, _lib.ptr(o["dw"].t),
                                              _lib.ptr(o["ws"].t), o["ws"].nbytes, _lib.stream_ptr()) != 0 and "multiple of 8" in _lib.last_error()
    torch.cuda.synchronize()
    assert _same_bytes(o["h"].t, second["h"].t) and _same_bytes(o["dw"].t, second["dw"].t)


def test_gated_layer_autograd_and_an_fp32_input():
    D, F, M = 64, 72, 17
    c = _dev(ref.gated_case(M, D, F))
    dx, dw = train_ops.gated_linear_backward(c["x"], c["w"], c["dh"])
    x, w = c["x"].float().view(1, M, D).requires_grad_(), c["w"].clone().requires_grad_()
    h = train_ops.gated_linear(x, w)
    assert tuple(h.shape) == (1, M, F) and _same_bytes(h.detach()[0], train_ops.gated_linear_forward(c["x"], c["w"]))
    h.backward(c["dh"].view(1, M, F))
    assert x.grad.dtype == torch.float32 and torch.equal(x.grad[0], dx.float()) and _same_bytes(w.grad, dw)


def test_gated_layer_where_m_times_2f_passes_2_to_the_31():
    """D = 8, F = 2048, M = 2^19 + 40: u has M * 2F = 2^31 + 163840 elements and the GEMMs run in three blocks of rows. x is zero except in
    the first and the last 64 rows, so h, du and dx are exactly zero elsewhere and dW1 is the sum over those 128 rows: everything is
    checked against fp64 on the sampled rows at both ends. An index that wrapped at 2^31 would leave the last rows unwritten."""
    D, F, M, S = 8, 2048, (1 << 19) + 40, 64
    assert M * 2 * F > 2 ** 31
    ends = ref.gated_case(2 * S, D, F, seed=5)
    c = _dev(ends)
    x = torch.zeros(M, D, dtype=torch.float16, device=DEV)
    x[:S], x[-S:] = c["x"][:S], c["x"][S:]
    dh = torch.empty(M, F, dtype=torch.float16, device=DEV)
    dh.normal_(generator=torch.Generator(device=DEV).manual_seed(11))
    dh[:S], dh[-S:] = c["dh"][:S], c["dh"][S:]
    h = train_ops.gated_linear_forward(x, c["w"])
    dx, dw = train_ops.gated_linear_backward(x, c["w"], dh)
    torch.cuda.synchronize()
    exact, yard = ref.gated_torch(ends), ref.gated_torch(ends, dtype=torch.float16)
    sample = lambda t: torch.cat([t[:S], t[-S:]])      # noqa: E731
    _check("gated D=%d F=%d M=%d (both ends)" % (D, F, M), ref.GATED_NAMES, (sample(h), sample(dx), dw), exact, yard)
    assert int(torch.count_nonzero(h[S:-S])) == 0 and int(torch.count_nonzero(dx[S:-S])) == 0
    assert int(torch.count_nonzero(h[-S:])) > 0 and int(torch.count_nonzero(dx[-S:])) > 0


# ---- the whole encoder layer --------------------------------------------------------------------------------------------------------------------
LAYER_NAMES = ("y", "dx") + ref.LAYER_PARAMS


@functools.lru_cache(maxsize=None)
def _layer_refs(N, T, D, H, F, window):
    case = ref.layer_case(N, T, D, F)
    return case, ref.layer_torch(case, H, window, V5_ALPHA), ref.layer_torch(case, H, window, V5_ALPHA, dtype=torch.float16)


def _container(case, D, H, F, window):
    layer = TransformerEncoderLayer(D, H, F, V5_ALPHA, 0.3, attn_window=window)
    missing = layer.load_state_dict({k: case[k] for k in ref.LAYER_PARAMS}, strict=False)
    assert missing.missing_keys == ["deepnorm_alpha"] and not missing.unexpected_keys
    return layer.to(DEV)


@pytest.mark.parametrize("N,T,window", ((2, 40, (3, 5)), (1, 300, (127, 128))), ids=lambda v: str(v))
@pytest.mark.parametrize("D,H,F", ((128, 2, 256), (192, 3, 200)))
def test_encoder_layer_within_twice_the_yardstick(D, H, F, N, T, window):
    case, exact, yard = _layer_refs(N, T, D, H, F, window)
    layer = _container(case, D, H, F, window)
    x = case["x"].to(DEV).requires_grad_()
    y = attn.encoder_layer(layer, x)
    assert y.dtype == torch.float16 and tuple(y.shape) == (N, T, D)
    y.backward(case["dy"].to(DEV))
    torch.cuda.synchronize()
    params = dict(layer.named_parameters())
    assert sorted(params) == sorted(ref.LAYER_PARAMS)
    for name, p in params.items():
        assert p.dtype == torch.float32 and p.grad is not None and p.grad.dtype == torch.float32 and p.grad.shape == p.shape, name
    assert layer.deepnorm_alpha.grad is None and not layer.deepnorm_alpha.requires_grad and x.grad.dtype == torch.float16
    got = (y.detach(), x.grad) + tuple(params[k].grad for k in ref.LAYER_PARAMS)
    _check("layer N=%d T=%d D=%d H=%d F=%d %s" % (N, T, D, H, F, window), LAYER_NAMES, got, [exact[k] for k in LAYER_NAMES],
           [yard[k] for k in LAYER_NAMES])


def test_encoder_layer_gradients_accumulate_and_deepnorm_alpha_gets_none():
    N, T, D, H, F, window = 2, 40, 128, 2, 256, (3, 5)
    case, _, _ = _layer_refs(N, T, D, H, F, window)
    layer = _container(case, D, H, F, window)
    x = case["x"].to(DEV).float().requires_grad_()
    dy = case["dy"].to(DEV)
    attn.encoder_layer(layer, x).backward(dy)
    assert x.grad.dtype == torch.float32
    once = {k: p.grad.clone() for k, p in layer.named_parameters()}
    attn.encoder_layer(layer, x).backward(dy)
    for k, p in layer.named_parameters():
        assert torch.equal(p.grad, 2 * once[k]), k                                    # the same bytes twice, added by autograd
    assert layer.deepnorm_alpha.grad is None
    with torch.no_grad():                                                              # the buffer is read again once its value changes
        first = attn.encoder_layer(layer, x)
        layer.deepnorm_alpha.fill_(1.0)
        assert not torch.equal(attn.encoder_layer(layer, x), first)

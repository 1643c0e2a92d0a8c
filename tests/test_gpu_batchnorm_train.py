"""Batch-statistics BatchNorm behind a convolution, on the device (-m gpu): bh_batchnorm_train_forward / _backward and
bonito_amd.train_ops.batchnorm.

exact = fp64 torch.nn.functional.batch_norm(training=True) + activation under autograd; yardstick = the same in fp16 on the CPU
(tests/batchnorm_train_ref.py, pinned by tests/test_batchnorm_train_ref_cpu.py). With dist(a) = max|a - exact| / max|exact|, y, dz, dgamma
and dbeta must satisfy dist(kernel) <= 2 dist(yardstick); mean, rstd and the running statistics (fp32) are held against fp64 within the
bound the reference file derives from the order of summation. The clamp's mask is read from the device's stored y; where it does not
hold, y is the bound itself. Every case prints its ratios.

The rest is exact: padded channels are zero, equal bytes from call to call, untouched guard bytes around every output and the
workspace, null outputs and buffers, refused calls that launch nothing, 64-bit indexing where N L C passes 2^31."""
import functools

import pytest
import torch

import batchnorm_train_ref as ref
from bonito_amd import _lib, train_ops

pytestmark = pytest.mark.gpu

DEV = "cuda"
INF = float("inf")
F64 = torch.float64
GUARD = 512


class _Guarded:
    """A device tensor between two guard zones of GUARD bytes of 0xA5 (the payload starts 0xA5 too)."""

    def __init__(self, shape, dtype, like=None):
        n = 1
        for s in shape:
            n *= s
        self.nbytes = n * torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.full((self.nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        self.t = self.raw[GUARD:GUARD + self.nbytes].view(dtype).view(shape)
        if like is not None:
            self.t.copy_(like)

    def guards_intact(self):
        return bool((self.raw[:GUARD] == 0xA5).all()) and bool((self.raw[GUARD + self.nbytes:] == 0xA5).all())

    def payload_untouched(self):
        return bool((self.raw == 0xA5).all())


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@functools.lru_cache(maxsize=None)
def _case(N, L, C, pad=0, offset_channel=None, constant_channel=None, affine=True, tracked=True):
    """The case on its C - pad real channels (CPU, never modified) and the device's padded tensors: the channels behind carry noise in z
    and dy, which the layer must neither read into a statistic nor write anything but zeros for."""
    case = ref.bn_case(N, L, C - pad, offset_channel=offset_channel, constant_channel=constant_channel)
    if not affine:
        case.update(gamma=None, beta=None)
    if not tracked:
        case.update(running_mean=None, running_var=None)
    g = torch.Generator().manual_seed(5)
    wide = lambda t: torch.cat([t, torch.randn(N, L, pad, generator=g).half()], 2).contiguous() if pad else t      # noqa: E731
    dev = {"z": wide(case["z"]).to(DEV), "dy": wide(case["dy"]).to(DEV)}
    for name in ("gamma", "beta"):            # C long, NaN behind the real channels: never read
        dev[name] = None if case[name] is None else torch.cat([case[name], torch.full((pad,), float("nan"))]).to(DEV)
    return case, dev


@functools.lru_cache(maxsize=None)
def _refs(key, act, m_bytes, shape):
    """(want, yardstick, bounds) for a case and the device's mask, computed once on the CPU."""
    case = _case(*key)[0]
    m = torch.frombuffer(bytearray(m_bytes), dtype=torch.bool).reshape(shape)
    f = ref.formulas(case, act, m)
    want = {**{k: f[k] for k in ("mean", "rstd")}, **ref.exact(case, act, m)}
    bounds = ref.stat_bounds(case["z"], case["running_mean"], case["running_var"]) if case["running_mean"] is not None else \
        {k: v for k, v in ref.stat_bounds(case["z"], None, None).items()}
    return want, ref.yardstick(case, act, m), bounds


def _raw(key, act, clamp, time_major=False, dgamma=True, dbeta=True):
    """One forward and one backward through the library on guarded buffers -> the buffers."""
    N, L, C, pad = key[0], key[1], key[2], key[3] if len(key) > 3 else 0
    case, dev = _case(*key)
    Cp = C - pad
    lib, s = _lib.lib(), _lib.stream_ptr()
    nbytes = lib.bh_batchnorm_train_workspace(N, L, C)
    assert nbytes >= 2 * -(-(N * L) // ref.block_rows(N * L)) * C * 4
    lo, hi = (-INF, INF) if clamp is None else clamp
    os_n, os_t = (C, N * C) if time_major else (L * C, C)
    o = {"y": _Guarded((L, N, C) if time_major else (N, L, C), torch.float16), "dz": _Guarded((N, L, C), torch.float16),
         "mean": _Guarded((Cp,), torch.float32), "rstd": _Guarded((Cp,), torch.float32), "dgamma": _Guarded((Cp,), torch.float32),
         "dbeta": _Guarded((Cp,), torch.float32), "ws": _Guarded((nbytes,), torch.uint8)}
    tracked = case["running_mean"] is not None
    if tracked:
        o["running_mean"] = _Guarded((Cp,), torch.float32, case["running_mean"])
        o["running_var"] = _Guarded((Cp,), torch.float32, case["running_var"])
    dy = dev["dy"].permute(1, 0, 2).contiguous() if time_major else dev["dy"]
    _lib.check(lib.bh_batchnorm_train_forward(_lib.ptr(dev["z"]), _lib.ptr(dev["gamma"]), _lib.ptr(dev["beta"]),
                                              _lib.ptr(o["running_mean"].t) if tracked else None, _lib.ptr(o["running_var"].t) if tracked else None,
                                              N, L, C, Cp, ref.EPS, ref.MOMENTUM, _lib.BH_ACT[act], lo, hi, os_n, os_t, _lib.ptr(o["y"].t),
                                              _lib.ptr(o["mean"].t), _lib.ptr(o["rstd"].t), _lib.ptr(o["ws"].t), nbytes, s), "bh_batchnorm_train_forward")
    _lib.check(lib.bh_batchnorm_train_backward(_lib.ptr(dev["z"]), _lib.ptr(dev["gamma"]), _lib.ptr(dev["beta"]), _lib.ptr(o["mean"].t),
                                               _lib.ptr(o["rstd"].t), _lib.ptr(o["y"].t), _lib.ptr(dy), N, L, C, Cp, _lib.BH_ACT[act], lo, hi, os_n,
                                               os_t, _lib.ptr(o["dz"].t), _lib.ptr(o["dgamma"].t) if dgamma else None,
                                               _lib.ptr(o["dbeta"].t) if dbeta else None, _lib.ptr(o["ws"].t), nbytes, s), "bh_batchnorm_train_backward")
    torch.cuda.synchronize()
    return o


def _run(key, act="swish", clamp=None, time_major=False):
    """Run, then hold every output against its reference; -> (the buffers, the mask)."""
    N, L, C, pad = key[0], key[1], key[2], key[3] if len(key) > 3 else 0
    Cp = C - pad
    case = _case(*key)[0]
    o = _raw(key, act, clamp, time_major)
    for name in o:
        assert o[name].guards_intact(), name
    y = (o["y"].t.permute(1, 0, 2) if time_major else o["y"].t).cpu()
    dz = o["dz"].t.cpu()
    if pad:
        assert int(torch.count_nonzero(y[:, :, Cp:])) == 0 and int(torch.count_nonzero(dz[:, :, Cp:])) == 0
        assert not bool(torch.signbit(y[:, :, Cp:].float()).any())
    y, dz = y[:, :, :Cp].contiguous(), dz[:, :, :Cp].contiguous()
    m = ref.mask_of(y, clamp)
    if clamp is not None:                 # outside the mask y is the bound itself
        yf = y.float()
        assert bool(((yf == clamp[0]) | (yf == clamp[1]))[~m].all()) and 0 < int(m.sum()) < m.numel()
    want, yard, bounds = _refs(key, act, m.numpy().tobytes(), tuple(m.shape))
    got = {"y": y, "dz": dz, **{k: o[k].t.cpu() for k in o if k not in ("y", "dz", "ws")}}
    label = "bn N=%d L=%d C=%d%s %s%s%s" % (N, L, C, "(-%d)" % pad if pad else "", act, " clamp" if clamp else "", " tm" if time_major else "")
    for name in ref.NAMES:
        if want.get(name) is None:
            continue
        dk = ref.dist(got[name] * m if name == "y" else got[name], want[name])
        dy = ref.dist(yard[name], want[name])
        print("%s %-12s: dist(kernel) = %.3e  dist(yardstick) = %.3e  ratio = %.3f" % (label, name, dk, dy, dk / dy if dy > 0 else (0.0 if dk == 0 else INF)))
    for name in ref.STATS:
        if want.get(name) is not None:
            err = (got[name].to(F64) - want[name]).abs()
            print("%s %-12s: max error / bound = %.3f" % (label, name, float((err / bounds[name]).max())))
    assert ref.outside(got, want, yard, bounds, m) == []
    assert bool(torch.isfinite(dz.float()).all())
    return o, m


# ---- every shape ------------------------------------------------------------------------------------------------------------------------------
# C: one vector per row (256 rows in flight), two, a whole wave's worth of 16-byte vectors twice over, and 65 vectors (three rows in
# flight, 61 idle threads). (N, L): the smallest M the layer serves, rows inside one slot pass, several row passes, more than one block
# of rows (M = 5000: 79 blocks of 64, the last one of 8); (7, 20011): M = 140077 > 2048 * 64, blocks of 69 rows, the last one of 7.
@pytest.mark.parametrize("N,L", ((1, 2), (3, 5), (2, 257), (5, 1000)))
@pytest.mark.parametrize("C", (8, 16, 64, 520))
def test_every_shape_within_twice_the_yardstick(C, N, L):
    _run((N, L, C))


def test_more_rows_than_the_blocks_of_least_size_hold():
    assert ref.block_rows(7 * 20011) == 69 and (7 * 20011) % 69 != 0
    _run((7, 20011, 8))


# ---- every option -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", (None, ref.CLAMP))
@pytest.mark.parametrize("act", (None, "swish", "relu", "tanh"))
def test_every_activation_with_and_without_the_clamp(act, clamp):
    _run((3, 50, 16), act, clamp)
    _run((2, 257, 64), act, clamp, time_major=True)


def test_time_major_store_has_the_bytes_of_the_batch_major_one():
    a, b = _raw((3, 50, 16), "swish", ref.CLAMP), _raw((3, 50, 16), "swish", ref.CLAMP, time_major=True)
    assert _same_bytes(a["y"].t.permute(1, 0, 2), b["y"].t)
    for name in ("dz", "dgamma", "dbeta", "mean", "rstd", "running_mean", "running_var"):
        assert _same_bytes(a[name].t, b[name].t), name


@pytest.mark.parametrize("N,L,C", ((3, 5, 16), (2, 257, 64), (5, 1000, 520)))
def test_padded_channels_are_zero_and_touch_no_statistic(N, L, C):
    o, _ = _run((N, L, C, 4), "swish", ref.CLAMP)
    wide, _ = _case(N, L, C, 4)
    assert tuple(o["mean"].t.shape) == (C - 4,)                       # the guards behind C - 4 floats are intact: nothing was written there


def test_an_offset_channel_and_a_constant_channel():
    o, _ = _run((3, 50, 16, 0, 5, 9), "swish", None)
    assert abs(float(o["mean"].t[5]) - 8.0) < 0.05 and 10.0 < float(o["rstd"].t[5]) < 40.0
    assert float(o["mean"].t[9]) == pytest.approx(1.375, abs=1e-6) and float(o["rstd"].t[9]) == pytest.approx(ref.EPS ** -0.5, rel=1e-3)
    dz = o["dz"].t[:, :, 9].float()
    assert bool(torch.isfinite(dz).all())
    _run((5, 1000, 64, 0, 63, 0), "swish", ref.CLAMP)


def test_without_affine_parameters_and_without_running_buffers():
    _run((3, 50, 16, 0, None, None, False, True))
    _run((3, 50, 16, 0, None, None, True, False), "relu", ref.CLAMP)
    _run((2, 257, 64, 4, None, None, False, False), "tanh")


def test_equal_bytes_guard_bytes_and_null_gradients():
    for key in ((5, 1000, 520), (3, 5, 16, 4), (7, 20011, 8)):
        first, second = _raw(key, "swish", ref.CLAMP), _raw(key, "swish", ref.CLAMP)
        for o in (first, second):
            for name in o:
                assert o[name].guards_intact(), name
        for name in first:
            if name != "ws":
                assert _same_bytes(first[name].t, second[name].t) and bool(torch.isfinite(first[name].t.float()).all()), name
        no_g, no_b = _raw(key, "swish", ref.CLAMP, dgamma=False), _raw(key, "swish", ref.CLAMP, dbeta=False)
        assert no_g["dgamma"].payload_untouched() and _same_bytes(no_g["dbeta"].t, first["dbeta"].t) and _same_bytes(no_g["dz"].t, first["dz"].t)
        assert no_b["dbeta"].payload_untouched() and _same_bytes(no_b["dgamma"].t, first["dgamma"].t) and _same_bytes(no_b["dz"].t, first["dz"].t)


def test_refused_calls_launch_nothing():
    N, L, C = 3, 5, 16
    case, dev = _case(N, L, C)
    lib, s = _lib.lib(), _lib.stream_ptr()
    nbytes = lib.bh_batchnorm_train_workspace(N, L, C)
    o = {"y": _Guarded((N, L, C), torch.float16), "mean": _Guarded((C,), torch.float32), "rstd": _Guarded((C,), torch.float32),
         "rm": _Guarded((C,), torch.float32), "ws": _Guarded((nbytes,), torch.uint8), "dz": _Guarded((N, L, C), torch.float16)}
    o["rv"] = o["rm"]

    def fwd(N=N, L=L, C=C, Cp=C, eps=ref.EPS, mom=0.1, act=1, lo=-INF, hi=INF, os_n=L * C, os_t=C, ws=nbytes, z=dev["z"], beta=dev["beta"],
            rv=o["rv"].t, y=o["y"].t):
        return lib.bh_batchnorm_train_forward(_lib.ptr(z), _lib.ptr(dev["gamma"]), _lib.ptr(beta), _lib.ptr(o["rm"].t), _lib.ptr(rv), N, L, C, Cp,
                                              eps, mom, act, lo, hi, os_n, os_t, _lib.ptr(y), _lib.ptr(o["mean"].t), _lib.ptr(o["rstd"].t),
                                              _lib.ptr(o["ws"].t), ws, s)

    def bwd(**kw):
        k = dict(N=N, L=L, C=C, Cp=C, act=1, lo=-INF, hi=INF, os_n=L * C, os_t=C, ws=nbytes, dz=o["dz"].t)
        k.update(kw)
        return lib.bh_batchnorm_train_backward(_lib.ptr(dev["z"]), _lib.ptr(dev["gamma"]), _lib.ptr(dev["beta"]), _lib.ptr(dev["gamma"]),
                                               _lib.ptr(dev["beta"]), _lib.ptr(dev["z"]), _lib.ptr(dev["dy"]), k["N"], k["L"], k["C"], k["Cp"],
                                               k["act"], k["lo"], k["hi"], k["os_n"], k["os_t"], _lib.ptr(k["dz"]), None, None, _lib.ptr(o["ws"].t),
                                               k["ws"], s)

    for kw, text in ((dict(N=1, L=1), "more than one value per channel"), (dict(C=12, Cp=12), "multiple of 8"), (dict(C=2056, Cp=8), "multiple of 8"),
                     (dict(Cp=17), "C_param must be in 1..C"), (dict(Cp=0), "C_param must be in 1..C"), (dict(N=0), "must be positive"),
                     (dict(eps=0.0), "eps must be finite and > 0"), (dict(eps=INF), "eps must be finite and > 0"), (dict(mom=-0.1), "momentum must be in 0..1"),
                     (dict(mom=1.5), "momentum must be in 0..1"), (dict(act=7), "unknown activation 7"), (dict(lo=1.0, hi=-1.0), "is empty"),
                     (dict(os_t=12), "multiples of 8"), (dict(os_n=-16), "multiples of 8"), (dict(ws=nbytes - 1), "workspace of"),
                     (dict(z=dev["z"].view(-1)[4:]), "16-byte aligned"), (dict(beta=None), "gamma and beta come together"),
                     (dict(rv=None), "running_mean and running_var come together"), (dict(y=None), "null pointer")):
        assert fwd(**kw) != 0 and text in _lib.last_error(), (kw, _lib.last_error())
    for kw, text in ((dict(N=1, L=1), "more than one value per channel"), (dict(C=12, Cp=12), "multiple of 8"), (dict(act=-1), "unknown activation"),
                     (dict(os_n=4), "multiples of 8"), (dict(ws=16), "workspace of"), (dict(dz=None), "null pointer"),
                     (dict(dz=o["dz"].t.view(-1)[4:]), "16-byte aligned")):
        assert bwd(**kw) != 0 and text in _lib.last_error(), (kw, _lib.last_error())
    torch.cuda.synchronize()
    for name in o:
        assert o[name].payload_untouched(), name


# ---- the autograd function ----------------------------------------------------------------------------------------------------------------------
def test_autograd_hands_on_the_bytes_the_dtypes_and_the_running_statistics():
    key = (3, 50, 16, 4)
    case, dev = _case(*key)
    raw = _raw(key, "swish", ref.CLAMP, time_major=True)
    z = dev["z"].float().requires_grad_()                                                   # fp32 in: the gradient comes back as fp32
    gamma, beta = (torch.nan_to_num(dev[k]).clone().requires_grad_() for k in ("gamma", "beta"))
    rm, rv = case["running_mean"].to(DEV), case["running_var"].to(DEV)
    y = train_ops.batchnorm(z, gamma, beta, rm, rv, ref.MOMENTUM, ref.EPS, "swish", ref.CLAMP, time_major=True, channels=12)
    assert y.dtype == torch.float16 and tuple(y.shape) == (50, 3, 16) and _same_bytes(y, raw["y"].t)
    assert _same_bytes(rm, raw["running_mean"].t) and _same_bytes(rv, raw["running_var"].t)
    y.backward(dev["dy"].permute(1, 0, 2).contiguous())
    assert z.grad.dtype == torch.float32 and _same_bytes(z.grad.half(), raw["dz"].t)
    assert _same_bytes(gamma.grad[:12], raw["dgamma"].t) and _same_bytes(beta.grad[:12], raw["dbeta"].t)
    assert int(torch.count_nonzero(gamma.grad[12:])) == 0 and int(torch.count_nonzero(beta.grad[12:])) == 0
    assert _same_bytes(rm, raw["running_mean"].t)                                          # the backward updates nothing
    with torch.no_grad():                                                                   # ... and the forward does, under no_grad too
        train_ops.batchnorm(z, gamma, beta, rm, rv, ref.MOMENTUM, ref.EPS, "swish", ref.CLAMP, channels=12)
    assert not _same_bytes(rm, raw["running_mean"].t) and not _same_bytes(rv, raw["running_var"].t)
    frozen = train_ops.batchnorm(dev["z"], gamma.detach(), beta.detach(), None, None, activation="swish", channels=12)      # nothing asks for a gradient
    assert not frozen.requires_grad
    plain = train_ops.batchnorm(dev["z"].requires_grad_(False), None, None)
    assert tuple(plain.shape) == (3, 50, 16) and bool(torch.isfinite(plain.float()).all())


# ---- 64-bit indexing ------------------------------------------------------------------------------------------------------------------------------
def test_more_than_two_to_the_31_elements():
    """N L C = 4099 * 65537 * 8 > 2^31, no activation, no clamp: the statistics and the gradient sums against fp64 sums taken in chunks
    on the device, y and dz on sampled rows against the formulas. A stored fp16 value is its fp32 value rounded once (2^-11 relative); the
    fp32 value carries the statistics' error, far below that: 2^-10 |want| + 1e-4."""
    N, L, C = 4099, 65537, 8
    M = N * L
    assert M * C > 2 ** 31
    g = torch.Generator(device=DEV).manual_seed(11)
    z = torch.empty(N, L, C, dtype=torch.float16, device=DEV).normal_(0.25, 1.5, generator=g)
    dy = torch.empty(N, L, C, dtype=torch.float16, device=DEV).normal_(0.5, 1.0, generator=g)
    gamma = torch.linspace(0.5, 1.5, C, device=DEV)
    beta = torch.linspace(-0.3, 0.3, C, device=DEV)
    y, mean, rstd = train_ops.batchnorm_forward(z, gamma, beta)
    dz, dgamma, dbeta = train_ops.batchnorm_backward(z, gamma, beta, mean, rstd, y, dy)
    torch.cuda.synchronize()
    rows, drows = z.view(M, C), dy.view(M, C)
    chunks = [(lo, min(M, lo + (1 << 24))) for lo in range(0, M, 1 << 24)]
    mean64 = sum(rows[lo:hi].sum(0, dtype=F64) for lo, hi in chunks) / M
    var64 = sum(((rows[lo:hi].to(F64) - mean64) ** 2).sum(0) for lo, hi in chunks) / M
    rstd64 = (var64 + ref.EPS).rsqrt()
    db64 = sum(drows[lo:hi].sum(0, dtype=F64) for lo, hi in chunks)
    dg64 = sum((drows[lo:hi].to(F64) * (rows[lo:hi].to(F64) - mean64) * rstd64).sum(0) for lo, hi in chunks)
    u = ref.U32 * ref.depth(M)
    absmean = sum(rows[lo:hi].abs().sum(0, dtype=F64) for lo, hi in chunks) / M
    print("2^31: max |mean error| = %.3e (bound %.3e), max rstd error = %.3e" % (float((mean.to(F64) - mean64).abs().max()),
                                                                                 float((u * absmean).max()), float((rstd.to(F64) - rstd64).abs().max())))
    assert bool(((mean.to(F64) - mean64).abs() <= (ref.depth(M) + 1) * ref.U32 * absmean).all())
    dm = (ref.depth(M) + 1) * ref.U32 * absmean
    dv = (ref.depth(M) + 4) * ref.U32 * (var64 + dm * dm) + dm * dm
    assert bool(((rstd.to(F64) - rstd64).abs() <= rstd64 * (0.5 * dv / (var64 + ref.EPS) + 3 * ref.U32)).all())
    # sums of M terms of magnitude ~1 each: the same order of summation, |du| and |du xh| in place of |z|
    assert bool(((dbeta.to(F64) - db64).abs() <= (ref.depth(M) + 1) * ref.U32 * M * 1.5).all())
    assert bool(((dgamma.to(F64) - dg64).abs() <= (ref.depth(M) + 1) * ref.U32 * M * 1.5).all())
    pick = torch.tensor([0, 1, L - 1, L, M // 2 + 12345, (1 << 28) - 1, 1 << 28, (1 << 28) + 1, M - 2, M - 1], device=DEV)
    xh = (rows[pick].to(F64) - mean64) * rstd64
    want_y = gamma.to(F64) * xh + beta.to(F64)
    want_dz = gamma.to(F64) * rstd64 * (drows[pick].to(F64) - db64 / M - xh * dg64 / M)
    for name, got, want in (("y", y.view(M, C)[pick], want_y), ("dz", dz.view(M, C)[pick], want_dz)):
        err = (got.to(F64) - want).abs()
        print("2^31 %s on %d sampled rows: max error = %.3e" % (name, len(pick), float(err.max())))
        assert bool((err <= 2.0 ** -10 * want.abs() + 1e-4).all()), name

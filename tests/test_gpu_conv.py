"""Every convolution kernel and instance against the fp64 restatement of tests/conv_ref.py (run with -m gpu on MI355X).

One helper (`_run`) per call description: the input in a buffer with fp16 NaN in front of and behind it (a read outside poisons an output
even through a zero weight), the whole `out` allocation (16 halves in front, every row with its padding columns, 64 rows behind)
pre-filled with an fp16 NaN payload; the call under the named "conv_*" options, restored in `finally`; then (i) bh_conv1d_last_kernel()
is the instance the case names, (ii) EVERY writable element is within its a-priori bound of the fp64 value (compared on the device),
(iii) every other element still holds the sentinel bit for bit, (iv) a second run writes identical bytes. No share of elements is excused.

Which instance a case must land on is restated here (`_expect`) from the launcher's documented conditions (csrc/conv.hip), so a changed
dispatch condition fails these tests instead of silently turning a "weight-stationary" test into a test of the generic kernel.

Pruning rule (that of tests/test_gpu_linear.py). Where the full product of a table would be wasteful, two of its factors span a full grid
and the remaining ones (pad, activation, clamp, bias, layout, N, row stride, ...) cycle with the running index of the grid, each through
a list whose length is coprime to the grid's inner dimension where that matters; every kernel has a second grid over two OTHER factors
(lengths x channels, lengths x strides), and the epilogue matrix (activation x clamp x bias) is run in full on every kernel that has one."""
import pytest
import torch

import conv_ref as cr
from conv_ref import Call, lin_for
from bonito_amd import _lib

pytestmark = pytest.mark.gpu
INF = float("inf")
S35 = dict(lo=-0.5, hi=3.5)                      # the models' clamp: bites on data class "big"
IN1 = dict(lo=-0.25, hi=0.5)                     # a clamp inside (-1, 1): bites on data class "normal"
K_FIRST, K_WS384, K_WS96, K_F384, K_F96, K_DW = (_lib.CONV_KERNELS[k] for k in ("first", "ws_384", "ws_96", "front3_384", "front3_96", "dwconv"))
DEFAULTS = dict(conv_ws=1, conv_fs=1, conv_fuse=1, conv_lds_kb=64)
NAMES = {K_FIRST: "conv_first", K_WS384: "conv_ws<384>", K_WS96: "conv_ws<96>", K_F384: "conv_front3<384>", K_F96: "conv_front3<96>",
         K_DW: "dwconv"}
WORST = {}               # kernel code -> (worst err / bound, case): printed by the last test of the file


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


def _name(code):
    return NAMES.get(code) or "conv_igemm<NTT=%d,FS=%d>" % ((code - 100) // 10, code % 10)


def _lds_for(c, pw):
    return (((4 * pw - 1) * c.stride + c.K) * c.Cin + 40) * 2 + 16


def _expect(c, opts, bias_aligned=True):
    """The kernel the launchers must pick, restated from csrc/conv.hip: Cin == 1 -> conv_first; depthwise -> dwconv; the weight-stationary
    kernel for 384 / 96 channels with a padded K * Cin of 320 whose 256-position span fits 64 KiB, under "conv_ws" and with a null or
    16-byte aligned bias; else conv_igemm with the largest of 64 / 32 / 16 positions per wave whose span fits "conv_lds_kb" KiB (16 if
    none does), feature-split under "conv_fs" when Cout % 64 == 0."""
    if c.kind == "first":
        return K_FIRST
    if c.kind == "dw":
        return K_DW
    o = dict(DEFAULTS, **opts)
    kp = -(-c.K * c.Cin // 32) * 32
    if o["conv_ws"] and c.Cout in (384, 96) and kp == 320 and _lds_for(c, 64) <= 64 * 1024 and bias_aligned:
        return K_WS384 if c.Cout == 384 else K_WS96
    pw = 64
    while pw > 16 and _lds_for(c, pw) > o["conv_lds_kb"] * 1024:
        pw >>= 1
    return _lib.conv_igemm_code(pw // 16, bool(o["conv_fs"]) and c.Cout % 64 == 0)


def _lds_kb_for(c, ntt):
    """A "conv_lds_kb" under which the launcher takes NTT position tiles per wave for shape `c` (None: the shape cannot)."""
    for kb in (64, 150, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 96, 128):
        if _expect(c, dict(conv_ws=0, conv_lds_kb=kb)) // 10 == 10 + ntt and _lds_for(c, 16 * ntt) <= 160 * 1024:
            return kb
    return None


def _call(c, t, out_ptr):
    lib, p = _lib.lib(), _lib.ptr
    x = t["xbuf"].data_ptr() + 2 * cr.IN_GUARD
    os_n, os_t = c.abi_strides()
    if c.kind == "first":
        rc = lib.bh_conv1d_first(x, p(t["w"]), p(t["bias"]), out_ptr, c.N, c.Lin, c.Cout, c.K, c.stride, c.pad, c.act, c.lo, c.hi, os_n, os_t,
                                 _lib.stream_ptr())
    elif c.kind == "igemm":
        rc = lib.bh_conv1d(x, p(t["wpk"]), p(t["bias"]), out_ptr, c.N, c.Lin, c.Cin, c.Cout, c.K, c.stride, c.pad, c.act, c.lo, c.hi, os_n,
                           os_t, _lib.stream_ptr())
    else:
        rc = lib.bh_dwconv1d(x, p(t["w"]), out_ptr, c.N, c.Lin, c.Cout, c.K, c.stride, c.pad, _lib.stream_ptr())
    _lib.check(rc, "bh_conv1d* %r" % c)
    torch.cuda.synchronize()
    return lib.bh_conv1d_last_kernel()


def _inputs(c, seed=11, cls=None, x=None, misalign_bias=False):
    """Inputs of call `c` on the device; class "big" when the models' clamp is on (so that it bites). `x`: take these input values
    instead ([N][Lin][Cin] fp16: the bytes another kernel wrote). "igemm": the packed weights as conv_ref.pack restates the host packer
    (pinned against bh_conv1d_pack in tests/test_conv_ref_cpu.py)."""
    cls = cls or ("big" if c.hi == 3.5 else "normal")
    t = cr.make_inputs(c, dev(), seed, cls)
    if x is not None:
        t["x"], t["xbuf"] = x, c.alloc_in(x)
    if c.kind == "igemm":
        t["wpk"] = cr.pack(c, t["w"])
    if misalign_bias:
        assert c.bias
        hold = torch.zeros(c.Cout + 1, dtype=torch.float32, device=dev())
        hold[1:] = t["bias"]
        t["bias"] = hold[1:]
        assert t["bias"].data_ptr() % 16 == 4
    return t


def _set(opts):
    from bonito_amd import decode
    for k, v in opts.items():
        decode.set_option(k, v)


def _check(c, t, buf, ran, what):
    r = cr.verify(c, t, buf)
    print("%s %s" % (_name(ran), cr.message(c, r, what)))
    if r["worst"] < INF and r["worst"] > WORST.get(ran, (0.0, ""))[0]:
        WORST[ran] = (r["worst"], repr(c))
    assert cr.ok(r), cr.message(c, r, what)


def _run(c, opts=None, expect=None, t=None, out_shift=0, **kw):
    """-> (out allocation, inputs). out_shift: halves by which the whole allocation is moved off its 16-byte alignment."""
    opts = dict(opts or {})
    t = _inputs(c, **kw) if t is None else t
    aligned = t["bias"] is None or t["bias"].data_ptr() % 16 == 0
    want = _expect(c, opts, aligned)
    assert expect is None or expect == want, "the case names %s, the restated rule says %s" % (_name(expect), _name(want))
    bufs = [torch.cat((torch.full((out_shift,), cr.SENTINEL, dtype=torch.int16, device=dev()), c.alloc_out(dev()))) for _ in range(2)]
    try:
        _set(opts)
        ran = [_call(c, t, b.data_ptr() + 2 * (out_shift + cr.FRONT)) for b in bufs]
    finally:
        _set(DEFAULTS)
    what = ",".join("%s=%d" % kv for kv in sorted(opts.items()))
    assert ran == [want, want], "%s %r ran on %s, not on %s" % (what, c, _name(ran[0]), _name(want))
    _check(c, t, bufs[0][out_shift:], want, what)
    assert bool((bufs[0][:out_shift] == cr.SENTINEL).all())
    assert torch.equal(bufs[0], bufs[1]), "%s %r: a second run wrote other bytes" % (what, c)
    return bufs[0][out_shift:], t


def _lin(lout, K, stride, pad, extra=0):
    """lin_for with the largest pad <= `pad` under which `lout` positions exist (Lout = 1 under a pad of K - 1 has no input)."""
    while (lout - 1) * stride + K - 2 * pad + extra < 1:
        pad -= 1
    return lin_for(lout, K, stride, pad, extra), pad


def _epilogues():
    """activation x {no clamp, the models' clamp, a clamp inside (-1, 1)} x bias: in full."""
    return [dict(act=a, bias=b, **cl) for a in range(4) for cl in (dict(), S35, IN1) for b in (True, False)]


def _eid(e):
    return ",".join("%s=%s" % kv for kv in sorted(e.items()))


CYC = [dict(), dict(act=1, **S35), dict(act=2, bias=False), dict(act=3), dict(act=1, bias=False), dict(act=2, **IN1), dict(act=3, **S35, bias=False)]


# ---- conv_first ---------------------------------------------------------------------------------------------------------------------
def _first_cases():
    out, i = [], 0
    Ks, Ss, Ls, Cs = (1, 2, 5, 9, 19), (1, 2, 3, 6), (1, 255, 256, 257, 513), (1, 4, 6, 8, 16, 24, 344)
    for K in Ks:                                                   # K x stride in full
        for s in Ss:
            i += 1
            cout = Cs[i % 7]
            L, pad = _lin(Ls[i % 5], K, s, (0, K // 2, K - 1)[i % 3], extra=i % s)
            out.append(Call("first", (1, 3)[i % 2], L, 1, cout, K, s, pad, layout=("NTC", "TNC")[i // 2 % 2],
                            os_t=cout + (0, 8, 4)[i % 3] if cout % 4 == 0 else cout + (0, 1)[i % 2], **CYC[i % 7]))
    for lout in Ls:                                                # Lout x Cout in full
        for cout in Cs:
            i += 1
            K, s = Ks[i % 5], Ss[i % 4]
            L, pad = _lin(lout, K, s, (0, K // 2, K - 1)[i % 3], extra=i % s)
            out.append(Call("first", (1, 3)[i % 2], L, 1, cout, K, s, pad, layout=("NTC", "TNC")[i // 2 % 2], **CYC[i % 7]))
    return out


@pytest.mark.parametrize("c", _first_cases(), ids=repr)
def test_conv_first_shapes(c):
    _run(c, expect=K_FIRST)


@pytest.mark.parametrize("e", _epilogues(), ids=_eid)
@pytest.mark.parametrize("K,cout", [(5, 16), (5, 6), (9, 16)], ids=["k5_vec8", "k5_scalar", "k9_vec8"])
def test_conv_first_every_epilogue(K, cout, e):
    """K == 5 with swish is the unrolled fast path of the 16-byte store loop; K == 5 with any other activation, K == 5 on the scalar
    store path and K == 9 take the generic tap loop."""
    _run(Call("first", 3, lin_for(257, K, 1, K // 2), 1, cout, K, 1, K // 2, **e), expect=K_FIRST)


@pytest.mark.parametrize("why", ["on", "cout", "os_t", "os_n", "out_8_bytes"])
@pytest.mark.parametrize("act", [1, 2])
def test_conv_first_vec8_and_each_way_out_of_it(why, act):
    """The 16-byte store path needs Cout % 8 == 0, both output strides multiples of 8 and a 16-byte aligned `out`; each condition broken
    separately must give the same values through the scalar path, the padding columns and the shifted guards intact."""
    cout, os_t, lay, shift = {"on": (16, 24, "NTC", 0), "cout": (12, 16, "NTC", 0), "os_t": (16, 20, "NTC", 0), "os_n": (16, 20, "TNC", 0),
                              "out_8_bytes": (16, 24, "NTC", 4)}[why]
    c = Call("first", 3, lin_for(257, 5, 1, 2), 1, cout, 5, 1, 2, act=act, layout=lay, os_t=os_t, **S35)
    os_n, os_t_abi = c.abi_strides()
    assert (why in ("on", "out_8_bytes")) == (cout % 8 == 0 and os_n % 8 == 0 and os_t_abi % 8 == 0)
    _run(c, expect=K_FIRST, out_shift=shift)


# ---- conv_igemm ---------------------------------------------------------------------------------------------------------------------
# (Cin, K): k-step counts 1 (K * Cin = 24: zero-padded columns), 3, 4 (120: padded), 4, 5, 9, 8, 6
CIN_K = [(8, 3), (16, 5), (24, 5), (64, 2), (16, 9), (24, 12), (128, 2), (64, 3)]


def _igemm_cases():
    out, i = [], 0
    for ntt in (1, 2, 4):                                          # instance x Lout in full
        for fs in (0, 1):
            for lout in (64 * ntt - 1, 64 * ntt, 64 * ntt + 1, 64 * ntt + 17, 7):
                i += 1
                cin, K = CIN_K[i % 8]
                cout = (64, 128, 192)[i % 3] if fs or i % 4 == 0 else (4, 12, 16, 20, 60, 68)[i % 6]
                s = (1, 2, 3, 6)[i % 4]
                L, pad = _lin(lout, K, s, (0, K // 2, K - 1)[i % 3], extra=i % s)
                c = Call("igemm", (1, 3)[i % 2], L, cin, cout, K, s, pad, layout=("NTC", "TNC")[i // 2 % 2], os_t=cout + (0, 8, 4)[i % 3], **CYC[i % 7])
                if _lds_kb_for(c, ntt) is None:                    # the span of 64 * ntt positions at this stride is beyond 160 KiB: stride 1
                    L, pad = _lin(lout, K, 1, pad)
                    c = Call("igemm", c.N, L, cin, cout, K, 1, pad, layout=c.layout, os_t=c.os_t, **CYC[i % 7])
                out.append((c, ntt, fs and 1, dict(conv_ws=0, conv_fs=fs, conv_lds_kb=_lds_kb_for(c, ntt))))
    for j, (cin, K) in enumerate(CIN_K):                           # (Cin, K) x Cout in full, instances cycling
        for cout in (4, 12, 16, 20, 60, 64, 68, 128, 192):
            i += 1
            ntt, s = (1, 2, 4)[i % 3], (1, 2, 3, 6)[i % 4]
            if _lds_for(Call("igemm", 1, 4000, cin, cout, K, s, 0), 16 * ntt) > 160 * 1024:
                s = 1
            L, pad = _lin((64 * ntt + 17, 13, 64 * ntt + 1)[i % 3], K, s, (0, K // 2, K - 1)[i % 3], extra=i % s)
            c = Call("igemm", (3, 1)[i % 2], L, cin, cout, K, s, pad, layout=("NTC", "TNC")[i // 2 % 2], **CYC[i % 7])
            fs = 1 if cout % 64 == 0 and i % 5 else 0
            out.append((c, ntt, fs, dict(conv_ws=0, conv_fs=fs, conv_lds_kb=_lds_kb_for(c, ntt))))
    return out


@pytest.mark.parametrize("c,ntt,fs,opts", _igemm_cases(), ids=lambda v: repr(v) if isinstance(v, Call) else None)
def test_conv_igemm_instances_and_shapes(c, ntt, fs, opts):
    """All six instances: NTT through "conv_lds_kb", FS through "conv_fs" and Cout % 64; block-boundary lengths PB - 1, PB, PB + 1,
    PB + 17 and Lout < 16 on each; the FS four-step loop with (k-steps 5, 6, 9) and without (4, 8) a tail and not at all (1, 3)."""
    assert opts["conv_lds_kb"] is not None
    _run(c, opts, expect=_lib.conv_igemm_code(ntt, fs))


@pytest.mark.parametrize("e", _epilogues(), ids=_eid)
@pytest.mark.parametrize("cin,K,cout,fs", [(16, 5, 20, 0), (24, 5, 64, 1)], ids=["ntt1", "ntt4_fs"])
def test_conv_igemm_every_epilogue(cin, K, cout, fs, e):
    c = Call("igemm", 3, lin_for(273, K, 2, K // 2), cin, cout, K, 2, K // 2, layout="TNC", **e)
    ntt = 4 if fs else 1
    _run(c, dict(conv_lds_kb=_lds_kb_for(c, ntt)), expect=_lib.conv_igemm_code(ntt, fs))


@pytest.mark.parametrize("cout,fs", [(64, 1), (64, 0), (12, 0)])
def test_conv_igemm_above_64_kib_of_lds(cout, fs):
    """Cin = 128, K = 9, stride 2 under "conv_lds_kb" 150: a 133 KiB span, the launcher raises the kernel's LDS limit first."""
    c = Call("igemm", 1, lin_for(273, 9, 2, 4), 128, cout, 9, 2, 4, act=1, **S35)
    assert 64 * 1024 < _lds_for(c, 64) <= 150 * 1024
    _run(c, dict(conv_lds_kb=150, conv_fs=fs), expect=_lib.conv_igemm_code(4, fs))


def test_conv_igemm_tiny_values_round_into_the_subnormals():
    """Data class "tiny": outputs around 2^-13, where the fp16 spacing is the floor 2^-24 of the bound's ulp term."""
    _run(Call("igemm", 3, lin_for(65, 5, 1, 2), 16, 20, 5, 1, 2), cls="tiny")
    _run(Call("first", 3, lin_for(257, 5, 1, 2), 1, 16, 5, 1, 2), cls="tiny")


# ---- conv_ws ------------------------------------------------------------------------------------------------------------------------
WS_SHAPES = [(16, 19, 1), (16, 19, 5), (16, 19, 6), (16, 19, 7), (16, 20, 6), (32, 10, 1), (32, 10, 3), (8, 37, 6)]
WS_LOUT = (1, 15, 16, 17, 255, 256, 257)


def _ws_cases():
    out, i = [], 0
    for cin, K, s in WS_SHAPES:                                    # shape x channels in full
        for cout in (384, 96):
            i += 1
            L, pad = _lin(WS_LOUT[i % 7], K, s, (0, K // 2, K - 1)[i % 3], extra=i % s)
            out.append(Call("igemm", (1, 3)[i % 2], L, cin, cout, K, s, pad, layout=("TNC", "NTC")[i // 2 % 2], os_t=cout + (0, 8)[i % 2], **CYC[i % 7]))
    for lout in WS_LOUT:                                           # Lout x activation in full, on the models' conv3
        for act in range(4):
            i += 1
            L, pad = _lin(lout, 19, 6, 9, extra=i % 6)
            out.append(Call("igemm", (1, 3)[i % 2], L, 16, (384, 96)[i % 2], 19, 6, pad, act=act, bias=i % 3 != 0, layout="TNC",
                            **(dict(), S35, IN1)[i % 3]))
    return out


@pytest.mark.parametrize("c", _ws_cases(), ids=repr)
def test_conv_ws_and_generic_write_identical_bytes(c):
    """Every way the Kp == 320 rule is met inside the LDS limit, 384 and 96 channels; then "conv_ws" 0 on the same input: the generic
    kernel (whichever instance the rule names) passes the same check and writes the same bytes."""
    ws, t = _run(c, expect=K_WS384 if c.Cout == 384 else K_WS96)
    generic, _ = _run(c, dict(conv_ws=0), t=t)
    assert torch.equal(ws, generic)


@pytest.mark.parametrize("cout", [384, 96])
def test_conv_ws_is_not_taken_at_stride_8_nor_with_a_misaligned_bias(cout):
    c = Call("igemm", 3, lin_for(257, 19, 8, 9), 16, cout, 19, 8, 9, act=1, layout="TNC", **S35)
    assert _lds_for(c, 64) > 64 * 1024
    _run(c, expect=_lib.conv_igemm_code(2, cout % 64 == 0))
    c = Call("igemm", 3, lin_for(257, 19, 6, 9), 16, cout, 19, 6, 9, act=1, layout="TNC", **S35)
    ws, t = _run(c, expect=K_WS384 if cout == 384 else K_WS96)
    t2 = _inputs(c, misalign_bias=True)
    assert torch.equal(t2["bias"], t["bias"])
    generic, _ = _run(c, t=t2, expect=_lib.conv_igemm_code(4, cout % 64 == 0))
    assert torch.equal(ws, generic)


# ---- conv_front3 --------------------------------------------------------------------------------------------------------------------
def _front3_call(c1, c2, c3, t1, t2, t3, out_ptr):
    lib, p = _lib.lib(), _lib.ptr
    os_n, os_t = c3.abi_strides()
    rc = lib.bh_conv1d_front3(t1["xbuf"].data_ptr() + 2 * cr.IN_GUARD, c1.N, c1.Lin, p(t1["w"]), p(t1["bias"]), c1.K, c1.pad, c1.act, c1.lo, c1.hi,
                              p(t2["wpk"]), p(t2["bias"]), c2.K, c2.pad, c2.act, c2.lo, c2.hi, p(t3["wpk"]), p(t3["bias"]), c3.Cout, c3.K,
                              c3.stride, c3.pad, c3.act, c3.lo, c3.hi, out_ptr, os_n, os_t, _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _front3_layers(N, L3, K1, K2, K3, s3, p1, p2, p3, cout3, e1, e2, e3, layout="TNC", os_t=None):
    L2 = lin_for(L3, K3, s3, p3, extra=(L3 + K1) % s3)
    L1 = L2 + K2 - 1 - 2 * p2
    L0 = L1 + K1 - 1 - 2 * p1
    assert L0 >= 1 and L1 >= 1
    return (Call("first", N, L0, 1, 16, K1, 1, p1, **e1), Call("igemm", N, L1, 16, 16, K2, 1, p2, **e2),
            Call("igemm", N, L2, 16, cout3, K3, s3, p3, layout=layout, os_t=os_t, **e3))


def _front3_cases():
    out, i = [], 0
    E = [dict(act=1, **S35), dict(act=2), dict(act=3, bias=False), dict(act=0, **IN1), dict(act=1)]
    for K1 in (1, 3, 5, 8):                                        # K1 x K2 in full
        for K2 in (1, 5, 6):
            i += 1
            K3, s3 = (19, 20)[i % 2], (1, 5, 6, 7)[i % 4]
            out.append(((1, 3)[i % 2], (1, 16, 17, 255, 256, 257)[i % 6], K1, K2, K3, s3, (0, K1 // 2)[i % 2], (0, K2 // 2)[i // 2 % 2],
                        (0, K3 // 2)[i // 4 % 2], (384, 96)[i % 2], E[i % 5], E[(i + 1) % 5], E[(i + 2) % 5]))
    for L3 in (1, 16, 17, 255, 256, 257):                          # L3 x stride in full
        for s3 in (1, 5, 6, 7):
            i += 1
            K1, K2, K3 = (5, 1, 3, 8, 5)[i % 5], (5, 1, 6)[i % 3], (19, 20)[i // 2 % 2]
            out.append(((3, 1)[i % 2], L3, K1, K2, K3, s3, (K1 // 2, 0)[i % 2], (K2 // 2, 0)[i // 2 % 2], (K3 // 2, 0)[i // 4 % 2],
                        (96, 384)[i % 2], E[i % 5], E[(i + 3) % 5], E[(i + 1) % 5]))
    return out


def _f3id(v):
    return "N%d-L3_%d-K%d_%d_%d-s%d-p%d_%d_%d-C%d-a%d%d%d" % (v[:10] + (v[10]["act"], v[11]["act"], v[12]["act"]))


@pytest.mark.parametrize("case", _front3_cases(), ids=_f3id)
def test_conv_front3_equals_three_verified_kernels(case):
    """The intermediates of the fused kernel never leave LDS, so: (a) conv1, conv2, conv3 as three launches, each verified against fp64 ON
    THE BYTES THE PREVIOUS KERNEL WROTE (teacher-forced), (b) bh_conv1d_front3 on the same signal and weights writes conv3's allocation
    bit for bit - guards, padding columns and sentinel included - twice. The generic-tap conv1 path (K1 != 5), K2 != 5, strides other
    than 6, pads of 0, a last span chunk of 12 - 19 rows (every stride here) and L3 around the 16-position tile and the 256-position
    block. 96 channels run under "conv_fuse" 2 as the engine would need; the entry point itself does not read the option."""
    N, L3, K1, K2, K3, s3, p1, p2, p3, cout3, e1, e2, e3 = case
    c1, c2, c3 = _front3_layers(N, L3, K1, K2, K3, s3, p1, p2, p3, cout3, e1, e2, e3, os_t=cout3 + (0, 8)[L3 % 2])
    assert c3.Lout == L3 and c2.Lout == c3.Lin and c1.Lout == c2.Lin
    b1, t1 = _run(c1, expect=K_FIRST, seed=5)
    b2, t2 = _run(c2, seed=6, x=c1.out_view(b1)[c1.rows(dev()).reshape(-1), :16].reshape(N, c1.Lout, 16).view(torch.float16))
    b3, t3 = _run(c3, seed=7, x=c2.out_view(b2)[c2.rows(dev()).reshape(-1), :16].reshape(N, c2.Lout, 16).view(torch.float16),
                  expect=K_WS384 if cout3 == 384 else K_WS96)
    want = K_F384 if cout3 == 384 else K_F96
    fused = [c3.alloc_out(dev()) for _ in range(2)]
    try:
        _set(dict(conv_fuse=2))
        for f in fused:
            rc = _front3_call(c1, c2, c3, t1, t2, t3, f.data_ptr() + 2 * cr.FRONT)
            _lib.check(rc, "bh_conv1d_front3")
            assert _lib.lib().bh_conv1d_last_kernel() == want
    finally:
        _set(DEFAULTS)
    _check(c3, t3, fused[0], want, "fused")
    assert torch.equal(fused[0], b3), "the fused front end wrote other bytes than conv3 of the three kernels"
    assert torch.equal(fused[0], fused[1])


@pytest.mark.parametrize("why,kw", [("cout3_128", dict(cout3=128)), ("cout3_64", dict(cout3=64)), ("K2_7", dict(K2=7)), ("K1_9", dict(K1=9)),
                                    ("K3_21", dict(K3=21)), ("K3_18", dict(K3=18)), ("stride_8", dict(s3=8))])
def test_conv_front3_refuses_what_it_has_no_instance_for(why, kw):
    """Nonzero return, the predicate named in the message, nothing launched: `out` keeps the sentinel and the hook its last value."""
    a = dict(K1=5, K2=5, K3=19, s3=6, cout3=384)
    a.update(kw)
    c1, c2, c3 = _front3_layers(3, 17, a["K1"], a["K2"], a["K3"], a["s3"], a["K1"] // 2, a["K2"] // 2, a["K3"] // 2, a["cout3"],
                                dict(act=1), dict(act=1), dict(act=1))
    t1, t2, t3 = _inputs(c1), _inputs(c2), _inputs(c3)
    _run(Call("dw", 1, 8, 8, 8, 1))
    buf = c3.alloc_out(dev())
    rc = _front3_call(c1, c2, c3, t1, t2, t3, buf.data_ptr() + 2 * cr.FRONT)
    assert rc != 0 and "no instance" in _lib.last_error()
    assert bool((buf == cr.SENTINEL).all()) and _lib.lib().bh_conv1d_last_kernel() == K_DW


# ---- dwconv -------------------------------------------------------------------------------------------------------------------------
def _dw_cases():
    out, i = [], 0
    Ls = (1, 63, 64, 65, 129)
    for C in (8, 64, 72, 128, 264):                                # C x K in full
        for K in (1, 3, 33, 151):
            i += 1
            s = (1, 2)[i % 2] if K != 151 or i % 4 else 1
            L, pad = _lin(Ls[i % 5], K, s, (0, K // 2)[i // 2 % 2], extra=i % s)
            out.append(Call("dw", 3, L, C, C, K, s, pad))
    for lout in Ls:                                                # Lout x stride in full (x pad), on a partial channel block
        for s in (1, 2):
            for pad in (0, 16):
                out.append(Call("dw", 3, _lin(lout, 33, s, pad)[0], 72, 72, 33, s, _lin(lout, 33, s, pad)[1]))
    out.append(Call("dw", 3, lin_for(65, 151, 1, 75), 72, 72, 151, 1, 75))           # above 64 KiB of LDS at stride 1, partial channel block
    return out


@pytest.mark.parametrize("c", _dw_cases(), ids=repr)
def test_dwconv(c):
    """Channel blocks of 64 with a partial last one (C = 8, 72, 264), position blocks of 64; K = 151 takes more than 64 KiB of LDS."""
    _run(c, expect=K_DW)


def test_zz_worst_ratio_per_kernel():
    """Not a check of its own: prints the worst err / bound every kernel reached in this run (the table of DESIGN.md)."""
    for k in sorted(WORST):
        print("%-28s worst err / bound %.3f at %s" % (_name(k), WORST[k][0], WORST[k][1]))
    assert all(v[0] <= 1.0 for v in WORST.values())

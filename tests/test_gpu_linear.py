"""Every linear-layer GEMM kernel, epilogue and edge against the fp64 restatement of tests/linear_ref.py (run with -m gpu on MI355X).

One helper (`_run`) per call description: X / W / residual in buffers with their leading dimensions and NaN in every padding column, the
whole `out` allocation (16 halves in front, every addressable row, 64 rows behind) pre-filled with an fp16 NaN payload; the call under a
given "gemm_path" / "gemm_tile16"; then (i) bh_linear_last_kernel() is the kernel the case names, (ii) EVERY writable element is within
its a-priori bound of the fp64 value (compared on the device, in slabs), (iii) every other element still holds the sentinel bit for bit,
(iv) a second run writes identical bytes. No share of elements is excused anywhere.

Which kernel a case must land on is restated here (`_kernel`) from the launcher's documented rules, so a changed dispatch condition fails
these tests instead of silently turning a "four-wave" test into a test of another kernel.

Pruning rule. Where the full product of a table row would be wasteful, two of its factors span a full grid and the remaining ones (token
count, epilogue, bias) cycle with the sum of the grid indices, so every PAIR of values of any two factors of the row occurs (the shape
grids below: every (K, N), (K, M) and (N, M)). The epilogue matrix is run in full on every kernel except that `bias` alternates over the
(activation, mode) grid (both values occur with every activation and with every mode); every (kernel, activation, mode) triple, gated x
{bias, none}, residual x res_scale x activation and every fall-through pair of the four-wave launcher are present."""
import math

import pytest
import torch

import linear_ref as lr
from linear_ref import Call
from bonito_amd import _lib

pytestmark = pytest.mark.gpu
INF = float("inf")
QS = 0.125 * math.log2(math.e)
R = 2.4494897
S5 = dict(scale=5.0, lo=-4.5, hi=4.5)
WORST = {}               # kernel -> (worst err / bound, case id): printed by the last test of the file


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


def _kernel(c, path, tile16):
    """The kernel the launcher must pick (csrc/gemm.hip `launch`), restated: 1 = v1, 2 = v2, 3 = v3, 5 / 6 = v5 on 32x32x16 / 16x16x32."""
    tiles = -(-c.N // 256) * -(-c.M // 256)
    plain = c.scale == 1.0 and c.lo == -INF and c.hi == INF
    mode = (1 if c.res_scale is not None else 0) | (2 if c.rot is not None else 0) | (0 if plain else 4)
    instantiated = (mode == 0) if c.gated else {0: mode in (0, 1, 2, 4), 1: mode == 0, 2: mode in (0, 4), 3: False}[c.act]
    affine = c.row[0] <= 0 or c.row[0] % 256 == 0 or (c.row[0] == 1 and c.row[1] == 1)
    if (path in (0, 5) and c.K % 128 == 0 and c.K >= 384 and c.N % 256 == 0 and (tiles >= 512 or path == 5) and affine
            and (c.rot is None or c.rot[0] >= 256) and instantiated):
        return 6 if tile16 else 5
    if path in (0, 3) and c.K % 64 == 0 and c.N >= 256 and c.N % 16 == 0 and tiles >= 512:
        return 3
    return 2 if c.K % 32 == 0 and path != 1 else 1


def _call(c, t, buf):
    lib, p = _lib.lib(), _lib.ptr
    out = buf.data_ptr() + 2 * lr.FRONT
    if c.rot is not None:
        rc = lib.bh_linear_qkv_rotary(p(t["X"]), p(t["W"]), p(t["bias"]), out, c.M, c.N // 3, c.K, p(t["cs"]), c.rot[0], c.rot[1],
                                      _lib.stream_ptr())
    elif c.res_scale is not None:
        rc = lib.bh_linear_residual(p(t["X"]), p(t["W"]), p(t["bias"]), out, c.M, c.N, c.K, c.ldx, c.ldw, c.ldo, c.act, c.scale, c.lo, c.hi,
                                    c.gated, c.row[0], c.row[1], c.row[2], c.row[3], p(t["res"]), c.ldres, c.res_scale, _lib.stream_ptr())
    else:
        rc = lib.bh_linear(p(t["X"]), p(t["W"]), p(t["bias"]), out, c.M, c.N, c.K, c.ldx, c.ldw, c.ldo, c.act, c.scale, c.lo, c.hi,
                           c.gated, c.row[0], c.row[1], c.row[2], c.row[3], _lib.stream_ptr())
    _lib.check(rc, "bh_linear*")
    torch.cuda.synchronize()
    return lib.bh_linear_last_kernel()


def _run(c, path, tile16=1, expect=None, seed=11, inputs=None):
    from bonito_amd import decode
    expect = _kernel(c, path, tile16) if expect is None else expect
    assert expect == _kernel(c, path, tile16)
    t = lr.make_inputs(c, dev(), seed) if inputs is None else inputs
    buf, again = c.alloc_out(dev()), c.alloc_out(dev())
    try:
        decode.set_option("gemm_tile16", tile16)
        decode.set_option("gemm_path", path)
        ran = _call(c, t, buf)
        ran2 = _call(c, t, again)
    finally:
        decode.set_option("gemm_path", 0)
        decode.set_option("gemm_tile16", 1)
    what = "gemm_path %d, gemm_tile16 %d:" % (path, tile16)
    assert ran == expect and ran2 == expect, "%s %r ran on kernel %d, not on %d" % (what, c, ran, expect)
    r = lr.verify(c, t, buf)
    print("kernel %d %s" % (ran, lr.message(c, r, what)))
    if r["worst"] < INF and r["worst"] > WORST.get(ran, (0.0, ""))[0]:
        WORST[ran] = (r["worst"], repr(c))
    assert r["bad"] == 0 and r["lost"] == 0, lr.message(c, r, what)
    assert torch.equal(buf, again), "%s %r: a second run wrote other bytes" % (what, c)
    return buf, t


# epilogues that cycle over the shape grids (gated needs N % 16 == 0: plain there otherwise)
CYCLE = [dict(), dict(act=1, bias=False), dict(act=2, **S5), dict(act=3, scale=5.0, bias=False), dict(gated=1), dict(res_scale=R),
         dict(act=1, lo=-0.1, hi=2.0)]


def _grid(Ks, Ns, Ms):
    out = []
    for i, K in enumerate(Ks):
        for j, N in enumerate(Ns):
            e = dict(CYCLE[(i * len(Ns) + j) % len(CYCLE)])
            if e.get("gated") and N % 16:
                e = dict(res_scale=1.0, act=2)
            out.append(Call(Ms[(i + j) % len(Ms)], N, K, **e))
    return out


NS, MS = (5, 8, 77, 80, 128, 136), (1, 15, 127, 128, 129, 300)


@pytest.mark.parametrize("c", _grid((8, 16, 24, 40, 72, 200, 1000), NS, MS), ids=repr)
def test_k_tails_v1(c):
    """v1 is the only kernel that takes K % 32 != 0: partly filled 8-half chunk rows, scalar store path at N % 16 != 0, token edges."""
    _run(c, 0, expect=1)
    _run(c, 1, expect=1)


@pytest.mark.parametrize("c", _grid((32, 64, 96, 160, 2048), NS, MS), ids=repr)
def test_shapes_v2(c):
    _run(c, 2, expect=2)
    _run(c, 0, expect=2)
    if c.K in (64, 96):
        _run(c, 1, expect=1)            # v1 without a K tail


def _m512(N, extra=37):
    """Token count that gives >= 512 tiles of 256 x 256 with a ragged last token tile."""
    nf = -(-N // 256)
    return (-(-512 // nf) - 1) * 256 + extra


V3_CYCLE = [dict(), dict(act=1, bias=False), dict(act=2, **S5), dict(gated=1), dict(res_scale=R), dict(act=3, scale=5.0)]


@pytest.mark.parametrize("c", [Call(_m512(N), N, K, **V3_CYCLE[(i * 3 + j) % 6]) for i, N in enumerate((256, 272, 320, 1040))
                               for j, K in enumerate((64, 192, 512))], ids=repr)
def test_shapes_v3(c):
    """The eight-wave 256 x 256 kernel: ragged last FEATURE tile (N = 272, 320, 1040), ragged last token tile."""
    _run(c, 3, expect=3)


V5_MS = (1, 255, 256, 257, 1007, 20000 + 9)
V5_CYCLE = [dict(), dict(act=2, **S5), dict(gated=1, bias=False), dict(res_scale=R), dict(act=1), dict(gated=1), dict(act=2), dict(lo=-2.0, hi=2.0)]


@pytest.mark.parametrize("tile16", [0, 1])
@pytest.mark.parametrize("c", [Call(M, (256, 768, 1536)[(i + j) % 3], K, **V5_CYCLE[(i * 6 + j) % 8]) for i, K in enumerate((384, 512, 640, 1024, 2048))
                               for j, M in enumerate(V5_MS)], ids=repr)
def test_shapes_v5(c, tile16):
    _run(c, 5, tile16, expect=6 if tile16 else 5)


@pytest.mark.parametrize("tile16", [0, 1])
def test_v5_is_the_automatic_choice_at_512_tiles(tile16):
    _run(Call(_m512(768, 9), 768, 384), 0, tile16, expect=6 if tile16 else 5)
    _run(Call(_m512(768, 9), 768, 384, act=3), 0, tile16, expect=3)           # no ReLU instance of the four-wave kernel: the eight-wave one


def _epilogues():
    out = []
    modes = (dict(), S5, dict(lo=-1.5, hi=2.5), dict(scale=5.0))
    for act in range(4):
        for k, mode in enumerate(modes):
            out.append(dict(act=act, bias=(act + k) % 2 == 0, **mode))
    out += [dict(gated=1), dict(gated=1, bias=False), dict(gated=1, **S5), dict(gated=1, bias=False, lo=-1.5, hi=2.5)]
    out += [dict(res_scale=rs, act=act, bias=act != 1) for rs in (1.0, R) for act in (0, 1, 2)]
    out += [dict(res_scale=R, gated=1), dict(res_scale=R, scale=5.0), dict(res_scale=1.0, act=2, **S5)]
    return out


# (kernel name, path, tile16, M, N, K)
EPI_KERNELS = [("v1", 1, 1, 300, 144, 72), ("v2", 2, 1, 300, 144, 96), ("v3", 3, 1, _m512(256), 256, 64), ("v5", 5, 0, 1007, 512, 384),
               ("v5t16", 5, 1, 1007, 512, 384)]


@pytest.mark.parametrize("e", _epilogues(), ids=lambda e: ",".join("%s=%s" % kv for kv in sorted(e.items())) or "plain")
@pytest.mark.parametrize("name,path,tile16,M,N,K", EPI_KERNELS, ids=[k[0] for k in EPI_KERNELS])
def test_every_epilogue_on_every_kernel(name, path, tile16, M, N, K, e):
    """Activation 0-3 x {plain, scale 5 + clamp, clamp only, scale only}, gated, residual x res_scale x activation, residual + gated. Under
    "gemm_path" 5 the (activation, mode) pairs the four-wave kernel has no instance of must land on the 128-tile LDS-DMA kernel (v2):
    tanh + residual, swish + scale, ReLU, gated + clamp, residual + scale, ... (`_kernel`; asserted in `_run`)."""
    c = Call(M, N, K, **e)
    want = {"v1": 1, "v2": 2, "v3": 3}.get(name)
    if want is None:
        want = _kernel(c, path, tile16)
        assert want in (2, 5, 6)
    _run(c, path, tile16, expect=want)


def test_four_wave_fall_through_pairs_by_name():
    """The launcher's fall-through combinations, literally: each must run on v2 under "gemm_path" 5, and the pair next to it on v5."""
    M, N, K = 1007, 512, 384
    for e, k in [(dict(act=2, res_scale=R), 2), (dict(act=1, scale=5.0), 2), (dict(gated=1, bias=False, lo=-1.5, hi=2.5), 2),
                 (dict(res_scale=R, scale=5.0), 2), (dict(act=3), 2),
                 (dict(act=2, **S5), 6), (dict(act=1), 6), (dict(gated=1, bias=False), 6), (dict(res_scale=R), 6), (dict(scale=5.0), 6)]:
        _run(Call(M, N, K, **e), 5, 1, expect=k)
    _run(Call(2 * 255 + 3, 1536, 384, rot=(255, QS)), 5, 1, expect=2)           # rot_T < 256
    _run(Call(2 * 256 + 3, 1536, 384, rot=(256, QS)), 5, 1, expect=6)
    _run(Call(3 * 48, 256, 384, row=(48, 1, 3, 43)), 5, 1, expect=2)            # row_div % 256 != 0
    _run(Call(3 * 256, 256, 384, row=(256, 1, 3, 251)), 5, 1, expect=6)


@pytest.mark.parametrize("gf", [1, 2, 3, 4, 5, 6, 8])
def test_four_wave_gemm_gf_rounds_down_to_a_power_of_two(gf):
    """ "gemm_gf" (feature tiles per block of the four-wave kernel's work order; eight feature tiles here, so 8 is not clamped): the kernel
    takes a power of two, the launcher rounds a request down to one. Every value passes the whole check of `_run`, writes the bytes of
    the default, and 3 / 5 / 6 write the bytes of 2 / 4 / 4."""
    from bonito_amd import decode
    c = Call(1007, 2048, 384, act=2, **S5)
    t = lr.make_inputs(c, dev(), 11)
    default, _ = _run(c, 5, 1, expect=6, inputs=t)
    rounded = 1 << (gf.bit_length() - 1)
    out = {}
    try:
        for g in sorted({gf, rounded}):
            decode.set_option("gemm_gf", g)
            out[g], _ = _run(c, 5, 1, expect=6, inputs=t)
    finally:
        decode.set_option("gemm_gf", 0)
    for g in out:
        assert torch.equal(out[g], default), "gemm_gf %d wrote other bytes than the default" % g
    assert torch.equal(out[gf], out[rounded]), "gemm_gf %d wrote other bytes than %d" % (gf, rounded)


ROT_TS = (1, 17, 255, 256, 300, 1667)


ROT_CASES = [(D, T, name, path, tile16, K) for name, path, tile16, K in (("v1", 1, 1, 72), ("v2", 2, 1, 64), ("v5", 5, 0, 384), ("v5t16", 5, 1, 384))
             for D in (64, 128, 512) for T in ROT_TS
             # (pruned: under "gemm_path" 5 the fall-through for 3 D % 256 != 0 is run at T = 17 and T = 300 only)
             if not name.startswith("v5") or D == 512 or T in (17, 300)]


@pytest.mark.parametrize("D,T,name,path,tile16,K", ROT_CASES, ids=["%s-D%d-T%d" % (c[2], c[0], c[1]) for c in ROT_CASES])
def test_rotary(D, T, name, path, tile16, K):
    """The fused rotary epilogue of Wqkv: M = 2 T + 3, so positions wrap inside a tile and M is no multiple of T. The four-wave kernel takes
    N = 3 D % 256 == 0 and T >= 256 only; anything else must fall through to v2."""
    c = Call(2 * T + 3, 3 * D, K, rot=(T, QS), bias=(ROT_TS.index(T) + D // 64) % 2 == 0)
    want = {"v1": 1, "v2": 2}.get(name)
    if want is None:
        want = (6 if tile16 else 5) if (D == 512 and T >= 256) else 2
    _run(c, path, tile16, expect=want)


@pytest.mark.parametrize("T,bias", [(300, True), (1667, False)])
def test_rotary_v3(T, bias):
    M = -(-(_m512(1536) + 1) // T) * T + 3
    _run(Call(M, 1536, 64, rot=(T, QS), bias=bias), 3, expect=3)


@pytest.mark.parametrize("name,path,tile16,N,K,e", [("v1", 1, 1, 77, 72, dict()), ("v2", 2, 1, 136, 96, dict(act=1)),
                                                    ("v5", 5, 0, 256, 384, dict(act=2, **S5)), ("v5t16", 5, 1, 256, 384, dict(act=2, **S5))])
@pytest.mark.parametrize("Np", (16, 48, 256, 512))
@pytest.mark.parametrize("nv", ("one", "minus5", "all"))
def test_row_remap(Np, nv, name, path, tile16, N, K, e):
    """The CRF head's remap (row_div, row_s_hi, row_s_lo, row_lim) = (Np, 1, T, Nv): (t, n)-major rows -> [n][t], padded batch rows
    dropped. The dropped rows' places are inside the allocation and must keep the sentinel."""
    T = 3
    Nv = {"one": 1, "minus5": Np - 5, "all": Np}[nv]
    c = Call(T * Np, N, K, row=(Np, 1, T, Nv), **e)
    want = {"v1": 1, "v2": 2}.get(name)
    if want is None:
        want = (6 if tile16 else 5) if Np % 256 == 0 else 2
    _run(c, path, tile16, expect=want)


@pytest.mark.parametrize("Nv", (1, 507))
def test_row_remap_v3(Nv):
    _run(Call(256 * 512, 256, 64, act=2, row=(512, 1, 256, Nv), **S5), 3, expect=3)


@pytest.mark.parametrize("name,path,N,K", [("v1", 1, 77, 72), ("v2", 2, 77, 96), ("v1", 1, 136, 200)])
def test_row_remap_with_residual_on_the_scalar_store_path(name, path, N, K):
    """N % 16 != 0 (per-element bias / residual guards, scalar stores) together with the remap: the residual is indexed by the input row."""
    _run(Call(5 * 48, N, K, act=2, row=(48, 1, 5, 43), res_scale=R), path, expect=1 if name == "v1" else 2)


LD_KERNELS = [("v1", 1, 1, 129, 136, 72), ("v2", 2, 1, 129, 136, 96), ("v3", 3, 1, _m512(320), 320, 64), ("v5", 5, 0, 1007, 512, 384),
              ("v5t16", 5, 1, 1007, 512, 384)]


@pytest.mark.parametrize("which", ("ldx", "ldw", "ldo", "ldres", "all", "gated_ldo", "all_clamp"))
@pytest.mark.parametrize("name,path,tile16,M,N,K", LD_KERNELS, ids=[k[0] for k in LD_KERNELS])
def test_leading_dimensions(name, path, tile16, M, N, K, which):
    """ldx = K + 8, ldw = K + 24, ldo = N + 8 (N / 2 + 8 gated), ldres = N + 8, separately and together: the padding columns of the inputs are
    NaN (never read), those of `out` must keep the sentinel (16-byte epilogue stores, whole-line stores of the four-wave kernel)."""
    e = {"ldx": dict(ldx=K + 8), "ldw": dict(ldw=K + 24), "ldo": dict(ldo=N + 8), "ldres": dict(ldres=N + 8, res_scale=R),
         "all": dict(ldx=K + 8, ldw=K + 24, ldo=N + 8, ldres=N + 8, res_scale=R), "gated_ldo": dict(gated=1, ldo=N // 2 + 8, ldx=K + 8),
         "all_clamp": dict(ldx=K + 8, ldw=K + 24, ldo=N + 8, act=2, **S5)}[which]
    if which == "gated_ldo" and N % 16:
        N, e = N + 8, dict(gated=1, ldo=(N + 8) // 2 + 8, ldx=K + 8)           # (the gated epilogue needs N % 16 == 0)
    _run(Call(M, N, K, **e), path, tile16)


def test_ldres_must_be_a_multiple_of_8():
    """The epilogues read the residual in 16-byte vectors: ldres = N + 2 is rejected, nothing is launched, `out` keeps the sentinel."""
    c = Call(129, 136, 72, res_scale=1.0, ldres=144)
    t = lr.make_inputs(c, dev(), 3)
    buf = c.alloc_out(dev())
    rc = _lib.lib().bh_linear_residual(_lib.ptr(t["X"]), _lib.ptr(t["W"]), _lib.ptr(t["bias"]), buf.data_ptr() + 2 * lr.FRONT, c.M, c.N, c.K,
                                       c.ldx, c.ldw, c.ldo, 0, 1.0, -INF, INF, 0, 0, 0, 0, 0, _lib.ptr(t["res"]), c.N + 2, 1.0, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and "ldres" in _lib.last_error()
    assert bool((buf == lr.SENTINEL).all())


@pytest.mark.parametrize("name,path,tile16,M,N,K", [("v1", 1, 1, 1024, 512, 384), ("v1_ktail", 1, 1, 1024, 512, 200), ("v2", 2, 1, 1024, 512, 384),
                                                    ("v3", 3, 1, _m512(512), 512, 384), ("v5", 5, 0, 1024, 512, 384), ("v5t16", 5, 1, 1024, 512, 384)])
def test_layouts_exactly(name, path, tile16, M, N, K):
    """X with one 1.0 per row against an asymmetric W: every output is ONE W element exactly, so a permuted fragment row, a wrong swizzle or
    a transposed store is a wrong value, not noise. Bit equality on top of the bound."""
    c = Call(M, N, K, bias=False)
    m = torch.arange(M, device=dev())
    x = torch.zeros(M, K, dtype=torch.float16, device=dev())
    x[m, (m * 7) % K] = 1.0
    w = (((torch.arange(N * K, device=dev()).reshape(N, K) * 37) % 2039).float() / 16.0).half()
    t = {"X": x, "W": w, "bias": None, "res": None, "cs": None}
    buf, _ = _run(c, path, tile16, inputs=t)
    want = w[:, (m * 7) % K].T.contiguous()
    assert torch.equal(c.out_view(buf)[:M].view(torch.float16), want)


def test_zz_worst_ratio_per_kernel():
    """Not a check of its own: prints the worst err / bound every kernel reached in this run (the figures of DESIGN.md section 6)."""
    for k in sorted(WORST):
        print("kernel %d: worst err / bound %.3f at %s" % (k, WORST[k][0], WORST[k][1]))
    assert all(v[0] <= 1.0 for v in WORST.values())

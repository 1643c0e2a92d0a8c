"""Sliding-window attention on the device (-m gpu): `bh_attention_prerotated` (the two ring kernels), `bh_attention` (the four instantiations
of the general kernel) and the engine's choice between them, against the fp64 restatement tests/attention_ref.py.

TOLERANCE. Nothing is fixed in advance (the convention of tests/test_gpu_seqdist.py): per case, d16 = the largest distance between the
reference with fp16 rounding where the kernel stores fp16 (attention_ref's docstring lists the places) and the fp64 reference, on the SAME
inputs. The kernel is allowed 4 x d16 against the fp64 reference (it accumulates in fp32 in another order and uses the hardware exp2).
Every test prints d16 and the kernel's distance; the measured pairs are in DESIGN.md (parity table, "Attention").
A tolerance of that size must not hide a dropped or admitted key: in every probe case, 4 x d16 is asserted to lie below ONE TENTH of the
smallest change that taking out / putting in the probed key makes to the fp64 output (both figures come from the reference alone).

INPUTS (all seeded).
  gauss  q, k, v i.i.d. Gaussian, as the tests of tests/test_gpu_ops.py.
  edge   every query is a probe. Keys are near-orthogonal unit vectors (+-1/8 per feature; the first 8 features are +1/8 in every key, so a
         query along minus that direction scores every real key at a large negative value). v is distinctive per key (Gaussian), except
         feature 0, which is 3 for every key: the output's feature 0 is 3 whatever the weights, unless an all-zero staging row (a row before
         the chunk, behind it, or in the padding between chunks) takes weight. Query i carries the softmax mass onto ONE key, by
         (i + 2 n + 3 h) mod 6: offset -wl, +wr (must be seen: output ~ v of that key), -wl - 1, +wr + 1 (must NOT be seen, although its raw
         score is the largest by far), 0, and "zero" (the query along minus the common direction: any zero row that is let in dominates).
         A probe whose key would lie outside the chunk becomes a "zero" probe, so the rows at both chunk ends carry those.
  seam   multi-chunk streams of the version-2 ring kernel: Gaussian queries, unit keys, and |v| ~ 1e3 (finite) in the first and last four rows
         of every chunk. The first four queries of chunk n point at the last four keys of chunk n - 1, the last four at the first four keys
         of chunk n + 1: a key that leaks across a chunk seam moves the output by ~1e3 x its weight.

No test provokes a device fault: every rejection is a host-side argument check.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import attention_ref as ar
from bonito_amd import _lib, decode

pytestmark = pytest.mark.gpu

RING_LEFT, RING_RIGHT = 128, 144          # the windows the ring kernels serve (include/bonito_hip.h, bh_attention_prerotated)
KINDS = 6                                  # -wl, +wr, -wl-1, +wr+1, 0, zero


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def make_case(entry, kind, N, T, H, win, seed):
    """-> (qkv fp16 [N, T, 3, H, 64], probes). probes (None for gauss): dict of [N, T, H] arrays - `probe` (bool: the query is a probe),
    `jx` (column of the probed key if it must be seen, else -1), `pn`, `pt` (chunk and row of a probed key that must NOT be seen; pn = -1:
    an all-zero row). `entry` "ring": q, k as the kernel multiplies them (base-2 scores); "general": the kernel rotates and scales by 1/8, so
    the designed q, k are rotated BACK here (and rounded to fp16: the reference works from the rounded values, like the kernel)."""
    rng = np.random.default_rng(seed)
    if kind == "gauss":
        return (rng.standard_normal((N, T, 3, H, 64), dtype=np.float32) * 0.7).astype(np.float16), None
    wl, wr = win
    beta = 64.0 if entry == "ring" else 256.0           # score of the probed key: 64 (base 2) / 256 / 8 = 32 (natural)
    zneg = 1.0 if entry == "ring" else 2.0              # "zero" probes score every real key at -8 (base 2) / -8 (natural)
    k = (rng.integers(0, 2, (N, T, H, 64)).astype(np.float32) * 2 - 1) / 8
    k[..., :8] = 0.125
    common = np.zeros(64, np.float32)
    common[:8] = 0.125
    v = rng.standard_normal((N, T, H, 64), dtype=np.float32)
    n_i, t_i, h_i = np.meshgrid(np.arange(N), np.arange(T), np.arange(H), indexing="ij")
    jx = np.full((N, T, H), -1)
    pn = np.full((N, T, H), -1)
    pt = np.zeros((N, T, H), int)
    if kind == "edge":
        v[..., 0] = 3.0
        kidx = (t_i + 2 * n_i + 3 * h_i) % KINDS
        off = np.array([-wl, wr, -wl - 1, wr + 1, 0, 0])[kidx]
        tgt = t_i + off
        zero = (kidx == 5) | (tgt < 0) | (tgt >= T)
        tg = np.where(zero, 0, tgt)
        q = np.where(zero[..., None], -beta * zneg * common, beta * k[n_i, tg, h_i])
        seen = ~zero & np.isin(kidx, (0, 1, 4))
        jx = np.where(seen, tg, -1)
        unseen = ~zero & ~seen
        pn = np.where(unseen, n_i, -1)
        pt = np.where(unseen, tg, 0)
        probe = np.ones((N, T, H), bool)
    else:
        assert kind == "seam" and T >= 8 and N >= 2
        q = rng.standard_normal((N, T, H, 64), dtype=np.float32) * 0.7
        ends = (np.arange(T) < 4) | (np.arange(T) >= T - 4)
        v[:, ends] *= 1000.0
        back = (t_i < 4) & (n_i > 0)                    # -> key T - 1 - t of the chunk before
        fwd = (t_i >= T - 4) & (n_i < N - 1)            # -> key T - 1 - t (0 .. 3) of the chunk behind
        probe = back | fwd
        pn = np.where(back, n_i - 1, np.where(fwd, n_i + 1, -1))
        pt = np.where(probe, T - 1 - t_i, 0)
        q = np.where(probe[..., None], beta * k[np.where(probe, pn, 0), pt, h_i], q)
    if entry == "general":
        q, k = ar.rotate(q, inverse=True), ar.rotate(k, inverse=True)
    qkv = np.stack([q, k, v], axis=2).astype(np.float16)
    return qkv, {"probe": probe, "jx": jx, "pn": pn, "pt": pt}


def reference(entry, qkv, win, probes, pairs):
    """-> (fp64 reference [N, T, H*64] (NaN outside `pairs`), d16, smallest probe effect or None)"""
    fn = ar.bh_attention if entry == "general" else ar.bh_attention_prerotated
    ref = fn(qkv, win, pairs=pairs)
    r16 = fn(qkv, win, storage_fp16=True, pairs=pairs)
    d16 = float(np.nanmax(np.abs(r16 - ref)))
    if probes is None:
        return ref, d16, None
    N, T, _, H, _ = qkv.shape
    mask = ar.visible(T, win)
    smallest = np.inf
    cache = {}

    def pair(n, h):
        if (n, h) not in cache:
            if len(cache) > 8:
                cache.clear()
            cache[(n, h)] = ar.pair_inputs(entry, qkv, n, h)
        return cache[(n, h)]
    for n, h in pairs:
        q, k, v = pair(n, h)
        pn, pt = probes["pn"][n, :, h], probes["pt"][n, :, h]
        kx, vx = np.zeros_like(k), np.zeros_like(v)              # default: an all-zero row
        for m in np.unique(pn[pn >= 0]):
            rows = pn == m
            _, km, vm = pair(int(m), h)
            kx[rows], vx[rows] = km[pt[rows]], vm[pt[rows]]
        eff = ar.probe_effects(q, k, v, mask, probes["jx"][n, :, h], kx, vx, base2=entry == "ring")
        sel = probes["probe"][n, :, h]
        if sel.any():
            smallest = min(smallest, float(eff[sel].min()))
    return ref, d16, smallest


def check_decisive(name, d16, smallest):
    if smallest is not None:
        assert 4 * d16 < smallest / 10, "%s: tolerance 4 x d16 = %.3e is not below a tenth of the smallest probe effect %.3e" % (
            name, 4 * d16, smallest)


def checked_pairs(N, T, H, entry):
    """All (chunk, head) pairs; for the 1667-token cases a seeded subset: the first and last chunk of every workgroup's stream (version-2
    ring kernel: chunks per workgroup = ceil(N / (CUs / heads))) with two heads each, topped up to at least a quarter of all pairs."""
    pairs = ar.all_pairs(N, H)
    if T < 1667 or len(pairs) <= 4:
        return pairs
    rng = np.random.default_rng(N * T + H)
    cus = torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256
    cols = max(cus // H, 1)
    cpw = (N + cols - 1) // cols
    chunks = sorted({c for g in range(0, N, cpw) for c in (g, min(g + cpw, N) - 1)})
    sub = {(c, int(h)) for c in chunks for h in rng.choice(H, size=min(2, H), replace=False)}
    rest = [p for p in pairs if p not in sub]
    rng.shuffle(rest)
    while 4 * len(sub) < len(pairs):
        sub.add(tuple(rest.pop()))
    return sorted(sub)


def distance(out, ref):
    """Largest |kernel - reference| over the checked pairs (NaN in `ref` = not checked); a NaN of the kernel anywhere is an error."""
    got = out.float().cpu().numpy().astype(np.float64).reshape(ref.shape)
    assert not np.isnan(got).any(), "the kernel left NaN in the output (rows not written, or 0 x inf)"
    return float(np.nanmax(np.abs(got - ref)))


def _ring_call(qd, N, T, H, win, head_dim=64):
    out = torch.full((max(N * T, 1), 64 * max(H, 1)), float("nan"), dtype=torch.float16, device=dev())
    rc = _lib.lib().bh_attention_prerotated(_lib.ptr(qd), _lib.ptr(out), N, T, H, head_dim, win[0], win[1], _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


def _rot_table(T, dim=64):
    tab = np.zeros((max(T, 1), dim // 2, 2), np.float32)
    _lib.check(_lib.lib().bh_rotary_table(max(T, 1), dim, tab.ctypes.data_as(C.c_void_p)), "rotary_table")
    return torch.from_numpy(tab)


def _general_call(qd, tab, N, T, H, win, head_dim=64):
    out = torch.full((max(N * T, 1), 64 * max(H, 1)), float("nan"), dtype=torch.float16, device=dev())
    rc = _lib.lib().bh_attention(_lib.ptr(qd), _lib.ptr(out), _lib.ptr(tab), N, T, H, head_dim, win[0], win[1], _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


def _assert_rejected(rc, out, win):
    assert rc != 0, "window %s accepted" % (win,)
    msg = _lib.last_error()
    assert str(win[0]) in msg and str(win[1]) in msg, "the message does not name the window %s: %r" % (win, msg)
    assert torch.isnan(out).all().item(), "a rejected call wrote to the output"


# ---- Sweep A: the ring entry --------------------------------------------------------------------------------------------------------
# (kind, N, T, H, window)  # the axis the case is there for
RING_CASES = [
    ("edge", 1, 1, 1, (0, 0)),            # T = 1; window (0, 0): one key per query, d16 = 0 - the kernel must be exact
    ("edge", 1, 15, 2, (128, 0)),         # T = 15 (< one tile); corner (128, 0)
    ("edge", 1, 16, 1, (0, 128)),         # T = 16 (P = T); corner (0, 128)
    ("edge", 2, 17, 1, (128, 128)),       # T = 17 (P = 32); corner (128, 128)
    ("gauss", 1, 143, 2, (127, 128)),     # T = 143; the reference window, Gaussian
    ("edge", 1, 144, 1, (0, 144)),        # T = 144; corner (0, 144): the widest right side
    ("edge", 1, 145, 2, (112, 144)),      # T = 145; (112, 144): wl + wr = 256 with wr at its limit
    ("edge", 1, 191, 1, (1, 143)),        # T = 191 (one short of a block of 192); (1, 143)
    ("edge", 1, 192, 1, (128, 144)),      # T = 192 (exactly one block); the far corner (128, 144)
    ("edge", 1, 193, 2, (0, 144)),        # T = 193 (one query in the second block of 192)
    ("edge", 1, 127, 1, (128, 0)),        # T = 127 (block of 128, minus one)
    ("edge", 1, 128, 1, (0, 128)),        # T = 128 (exactly one block of 128)
    ("edge", 1, 129, 1, (127, 128)),      # T = 129; the reference window on probes (every tile of the short chunk is partial or empty)
    ("edge", 1, 383, 2, (112, 144)),      # T = 383: the last length with eight waves chosen automatically
    ("edge", 1, 384, 2, (128, 144)),      # T = 384: the first with twelve
    ("gauss", 2, 383, 1, (0, 144)),       # Gaussian at the right-hand limit
    ("edge", 1, 1000, 2, (127, 128)),     # T = 1000: the straight-line path of version 2 (interior blocks) on probes
    ("gauss", 2, 1000, 8, (127, 128)),    # the production shape, Gaussian
    ("edge", 1, 1000, 1, (1, 143)),       # long chunk, (1, 143): the window slides over the ring wrap
    ("edge", 1, 1000, 1, (128, 128)),     # long chunk, (128, 128)
    ("edge", 1, 1000, 1, (0, 0)),         # long chunk, (0, 0): every tile but one empty
    ("gauss", 9, 1667, 8, (127, 128)),    # T = 1667 (P = 1680), Gaussian; a seeded quarter of the (chunk, head) pairs
    ("edge", 2, 1667, 1, (128, 144)),     # T = 1667 on probes at the far corner, all pairs
    ("seam", 70, 193, 8, (127, 128)),     # N = 70 at 8 heads: three chunks per workgroup, the last workgroup has one; P = 208 != T
    ("seam", 130, 129, 8, (128, 144)),    # N = 130 at 8 heads: five chunks per workgroup; P = 144
    ("seam", 300, 145, 1, (0, 144)),      # N = 300 at one head: two chunks per workgroup
    ("seam", 70, 144, 8, (112, 144)),     # P = T: the neighbour's rows touch this chunk's in the ring
    ("seam", 130, 17, 8, (127, 128)),     # chunks far shorter than the window: a dozen chunks are in the ring at once
    ("seam", 300, 16, 1, (128, 144)),     # the same with P = T = 16
    ("edge", 70, 100, 8, (128, 144)),     # edge probes (zero rows!) inside a multi-chunk stream
    # beyond the served range (wr > 144) but inside the guard of the first version of this entry: rejected, or right
    ("edge", 1, 1000, 1, (0, 145)),       # one key too many on the right
    ("edge", 1, 193, 1, (0, 145)),        # the same in a short chunk
    ("edge", 1, 384, 2, (16, 160)),       # (16, 160)
    ("edge", 2, 1000, 2, (64, 192)),      # (64, 192)
    ("gauss", 2, 400, 2, (64, 192)),      # (64, 192), Gaussian
    ("edge", 1, 1000, 1, (0, 256)),       # (0, 256)
    ("edge", 1, 383, 1, (1, 255)),        # (1, 255)
    ("seam", 70, 333, 8, (16, 160)),      # (16, 160) in a multi-chunk stream
]
RING_CONFIGS = [(2, 0), (2, 8), (2, 12), (1, 0), (1, 8), (1, 12)]          # (attn_version, attn_waves)


@pytest.mark.parametrize("kind,N,T,H,win", RING_CASES, ids=lambda x: str(x).replace(" ", ""))
def test_ring_entry_against_fp64(kind, N, T, H, win):
    """bh_attention_prerotated, both kernel versions, wave counts automatic / 8 / 12 (RING_CASES says which axis each case is there for).
    Windows with wr > 144 are not served by the ring kernels (a wave's 18 key tiles end 144 keys right of its last query): the entry
    must reject them and leave the output alone. Until it did, such a call succeeded with every key beyond q + 144 dropped - measured on
    MI355X on that library (version 2, automatic waves; kernel distance against a tolerance 4 x d16 of 3.9e-3): (0, 145) 5.4 at T = 1000 and
    2.8 at T = 193, (16, 160) 4.9, (64, 192) 5.1 on probes and 1.8 on Gaussian inputs, (0, 256) 5.0, (1, 255) 4.1, and 1.4e3 (tolerance 4.0)
    in the (16, 160) seam case. (128, 144) was refused by that library (its guard read wl + wr <= 256) although the kernels serve it.
    Measured on MI355X (d16 / largest kernel distance over the six configurations): see DESIGN.md, parity table, "Attention"."""
    name = "ring %s N%d T%d H%d %s" % (kind, N, T, H, win)
    qkv, probes = make_case("ring", kind, N, T, H, win, seed=N * 7919 + T * 31 + H + win[0] * 3 + win[1])
    qd = torch.from_numpy(qkv).to(dev()).reshape(N * T, 3 * H * 64).contiguous()
    served = win[0] <= RING_LEFT and win[1] <= RING_RIGHT
    ref = None
    try:
        for version, waves in RING_CONFIGS:
            decode.set_option("attn_version", version)
            decode.set_option("attn_waves", waves)
            rc, out = _ring_call(qd, N, T, H, win)
            if rc != 0:
                assert not served, "%s: a served window was rejected: %s" % (name, _lib.last_error())
                _assert_rejected(rc, out, win)
                continue
            if ref is None:
                pairs = checked_pairs(N, T, H, "ring")
                ref, d16, smallest = reference("ring", qkv, win, probes, pairs)
                check_decisive(name, d16, smallest)
            dk = distance(out, ref)
            print("%s v%d w%d: d16 %.3e kernel %.3e%s" % (name, version, waves, d16, dk,
                                                          "" if smallest is None else " (smallest probe effect %.3e)" % smallest))
            assert served, "%s: accepted a window the ring kernels do not serve (kernel distance %.3e, tolerance %.3e)" % (name, dk, 4 * d16)
            assert dk <= 4 * d16, (name, version, waves, dk, d16)
    finally:
        decode.set_option("attn_version", 2)
        decode.set_option("attn_waves", 0)


# ---- Sweep B: the general entry -----------------------------------------------------------------------------------------------------
def need_tiles(win):
    return (16 + win[0] + win[1] + 15) // 16          # bh_k_attention: key tiles one wave can see -> attention_kernel<6 | 10 | 18 | 26>


# (kind, N, T, H, window, need)  # T >= 3 x (wl + wr + 16) unless the case is there for T
GENERAL_CASES = [
    ("edge", 2, 290, 2, (40, 40), 6),          # <6> at its upper boundary, symmetric
    ("edge", 1, 290, 1, (80, 0), 6),           # ... one-sided left
    ("edge", 1, 290, 1, (0, 80), 6),           # ... one-sided right
    ("edge", 2, 300, 2, (40, 41), 7),          # <10> at its lower boundary: the instantiation no test launched before
    ("gauss", 2, 300, 2, (41, 40), 7),
    ("edge", 1, 291, 1, (0, 81), 7),
    ("edge", 1, 291, 1, (81, 0), 7),
    ("edge", 2, 485, 2, (72, 72), 10),         # <10> at its upper boundary
    ("edge", 1, 490, 1, (144, 0), 10),
    ("gauss", 1, 490, 2, (0, 144), 10),
    ("edge", 2, 483, 1, (72, 73), 11),         # <18> at its lower boundary
    ("edge", 1, 485, 1, (0, 145), 11),         # (also the first window the ring entry hands over)
    ("edge", 1, 870, 2, (136, 136), 18),       # <18> at its upper boundary
    ("edge", 1, 865, 1, (0, 272), 18),
    ("gauss", 2, 1000, 2, (127, 128), 17),     # the reference window on this kernel (`attn_ring` 0)
    ("edge", 1, 871, 2, (136, 137), 19),       # <26> at its lower boundary
    ("edge", 1, 870, 1, (273, 0), 19),
    ("edge", 1, 1250, 2, (200, 200), 26),      # <26> at its upper boundary, the window slides (the T = 64 case below cannot show that)
    ("edge", 1, 1250, 1, (400, 0), 26),
    ("edge", 1, 1251, 1, (0, 400), 26),
    ("gauss", 1, 1250, 2, (200, 200), 26),
    ("edge", 1, 800, 2, (64, 192), 17),        # the windows the engine now lowers onto this kernel
    ("edge", 1, 700, 1, (0, 200), 14),
    ("edge", 1, 1000, 1, (200, 100), 20),
    ("edge", 1, 1, 1, (0, 0), 1),              # T = 1
    ("edge", 2, 17, 1, (40, 41), 7),           # T = 17
    ("edge", 1, 129, 2, (136, 137), 19),       # T = 129: one query in the second workgroup (QB = 128)
    ("edge", 1, 128, 1, (72, 72), 10),         # T = 128: exactly one workgroup
    ("gauss", 2, 64, 1, (200, 200), 26),       # the wide case of tests/test_gpu_ops.py: every query sees the whole chunk
]


@pytest.mark.parametrize("kind,N,T,H,win,need", GENERAL_CASES, ids=lambda x: str(x).replace(" ", ""))
def test_general_entry_against_fp64(kind, N, T, H, win, need):
    """bh_attention: each of attention_kernel<6 | 10 | 18 | 26> on both sides of its boundary (need = 6 | 7, 10 | 11, 18 | 19, 26; 27 is
    rejected, see the rejection test), symmetric and one-sided windows, long enough for the window to slide. The output buffer is pre-filled
    with NaN and must come back without one. Measured on MI355X: DESIGN.md, parity table, "Attention"."""
    assert need_tiles(win) == need
    name = "general %s N%d T%d H%d %s need %d" % (kind, N, T, H, win, need)
    qkv, probes = make_case("general", kind, N, T, H, win, seed=N * 104729 + T * 31 + H + win[0] * 3 + win[1])
    ref, d16, smallest = reference("general", qkv, win, probes, ar.all_pairs(N, H))
    check_decisive(name, d16, smallest)
    qd = torch.from_numpy(qkv).to(dev()).reshape(N * T, 3 * H * 64).contiguous()
    rc, out = _general_call(qd, _rot_table(T).to(dev()), N, T, H, win)
    _lib.check(rc, "attention")
    dk = distance(out, ref)
    print("%s: d16 %.3e kernel %.3e%s" % (name, d16, dk, "" if smallest is None else " (smallest probe effect %.3e)" % smallest))
    assert dk <= 4 * d16, (name, dk, d16)


# ---- rejections ---------------------------------------------------------------------------------------------------------------------
def test_unserved_arguments_are_rejected_on_the_host_and_leave_the_output_alone():
    """Every window an entry does not serve, head_dim != 64, negative windows and empty problems: nonzero return, a message that names the
    window, the NaN-filled output untouched. All of these are argument checks in front of the launch."""
    N, T, H = 2, 40, 2
    qd = torch.zeros((N * T, 3 * H * 64), dtype=torch.float16, device=dev())
    tab = _rot_table(T).to(dev())
    for win in [(0, 145), (129, 0), (128, 145), (129, 144), (200, 200), (64, 192), (0, 256), (1, 255), (-1, 5), (5, -1), (-3, -3), (1 << 30, 1 << 30)]:
        _assert_rejected(*_ring_call(qd, N, T, H, win), win)
    for win in [(201, 200), (0, 401), (401, 0), (-1, 5), (5, -1), (1 << 29, 1 << 29)]:
        assert win[0] < 0 or win[1] < 0 or need_tiles(win) >= 27
        _assert_rejected(*_general_call(qd, tab, N, T, H, win), win)
    assert need_tiles((200, 200)) == 26 and need_tiles((201, 200)) == 27
    for call in (lambda **kw: _ring_call(qd, **kw), lambda **kw: _general_call(qd, tab, **kw)):
        for kw in [dict(N=N, T=T, H=H, win=(5, 5), head_dim=32), dict(N=N, T=T, H=H, win=(5, 5), head_dim=128),
                   dict(N=0, T=T, H=H, win=(5, 5)), dict(N=N, T=0, H=H, win=(5, 5)), dict(N=N, T=T, H=0, win=(5, 5))]:
            rc, out = call(**kw)
            assert rc != 0 and _lib.last_error() and torch.isnan(out).all().item(), kw


# ---- Sweep C: through the engine ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win,kernel", [((64, 192), "attention_kernel"), ((0, 200), "attention_kernel"), ((200, 100), "attention_kernel"),
                                        ((127, 128), "attention_ring_kernel")], ids=lambda x: str(x).replace(" ", ""))
def test_engine_lowers_each_window_onto_a_kernel_that_serves_it(win, kernel):
    """A two-layer transformer at 700 tokens with the given attn_window: engine output against oracle/nn_ref.py (fp32, and with fp16 rounding
    where the engine stores fp16), at the tolerance of tests/test_gpu_encoder.py for the tf_* fixtures (largest 2e-2, mean 3e-3 of the score
    range). The engine's layer description says which attention kernel serves the layers: windows outside the ring kernels' range (left
    <= 128, right <= 144) must be on the general kernel: that assertion is the one that proves the hand-over. The numbers alone do not -
    measured on MI355X on the library whose dispatch still put (64, 192) and (0, 200) on the ring kernel (keys beyond q + 144 dropped):
    largest / mean distance 7.4e-3 / 8.1e-4 for (64, 192) and 5.9e-2 / 5.0e-3 for (0, 200) against bounds of 1.3e-1 / 1.9e-2 and 1.1e-1 /
    1.6e-2 (with the served kernel: 5.2e-3 / 7.5e-4 and 5.2e-3 / 7.6e-4). A randomly initialised layer averages its values, and DeepNorm's
    residual carries most of the signal past the attention: the operator-level sweeps above are where a dropped key shows."""
    from bonito_amd import synthetic
    from bonito_amd.engine import HipEncoder
    from bonito_amd.transformer import Model
    from oracle import nn_ref
    torch.manual_seed(win[0] * 1000 + win[1])
    cfg = synthetic.transformer_model_config(d_model=128, nhead=2, dim_ff=256, depth=2, window=win, state_len=3, batchsize=3, chunksize=8400)
    model = Model(cfg).eval()
    with torch.no_grad():      # a freshly initialised layer attends almost uniformly, and an average over ~250 keys hardly notices 50 missing:
        for m in model.encoder.modules():          # sharpen the softmax (q and k rows of Wqkv x 4: scores x 16)
            if hasattr(m, "Wqkv"):
                m.Wqkv.weight[:2 * 128] *= 4.0
    nn_ref.round_params_to_half_(model.encoder)
    x = torch.randn(3, 1, 8400).half()
    enc = HipEncoder(model.encoder, batchsize=3, chunksize=8400)
    got = enc(x.cuda()).cpu().float()
    enc.check()
    layers = [line for line in enc.describe().splitlines() if " transformer " in line]
    figures = []
    for fp16 in (False, True):
        with torch.no_grad():
            want = nn_ref.forward(model.encoder, x.float(), expand_blanks=False, fp16=fp16)
        if want.shape != got.shape:
            want = want.permute(1, 0, 2)
        assert want.shape == got.shape
        d = (got - want).abs()
        rng = max(want.abs().max().item(), 1.0)
        figures.append((d.max().item(), d.mean().item(), rng))
        print("engine window %s vs oracle%s: max %.3e mean %.3e (range %.3g); layers: %s" % (
            win, " (fp16 storage)" if fp16 else "", d.max().item(), d.mean().item(), rng, [l.split("+")[-2].strip() for l in layers]))
    for dmax, dmean, rng in figures:
        assert dmax < 2e-2 * rng and dmean < 3e-3 * rng, (win, dmax, dmean, rng)
    assert len(layers) == 2 and all(("+ %s +" % kernel) in line for line in layers), layers

"""Plain fp64 restatement of the sliding-window attention operators (host only, numpy): the reference of tests/test_gpu_attention.py,
pinned by tests/test_attention_ref_cpu.py.

`windowed_attention(q, k, v, window)`: q, k, v [N, T, H, d]; key j of a chunk is visible to query i of the same chunk iff
i - wl <= j <= i + wr and 0 <= j < T; scores q . k (natural base) or base 2, softmax over the visible keys, P V. One (chunk, head) pair at
a time, whole [T, T] score matrix, nothing clever.

Two entry conventions sit on top of it:
  * `bh_attention(qkv, window)`            - packed qkv [N, T, 3, H, 64]; rotary as oracle/nn_ref.py::rotary (fp64 here), scale 1/8,
                                             natural base: the general kernel (`attention_kernel<NT>`).
  * `bh_attention_prerotated(qkv, window)` - q and k used as given (q already carries log2(e) / 8), softmax in base 2: the ring kernels.

`storage_fp16=True` rounds to fp16 exactly where the kernels store or feed fp16 (bonito_amd/csrc/attention.hip), everything else stays fp64:
  general kernel
    - rotated K                                       attention.hip:64-65
    - rotated Q times the scale 1/8                   attention.hip:99-100
    - the NORMALISED probabilities p / sum(p), the B fragment of the PV MFMAs (the row sum is taken over the unrounded p)
                                                      attention.hip:138-144,155-156
    - the output                                      attention.hip:176
  ring kernels (q, k arrive in fp16: nothing to round in front of the scores)
    - the UN-NORMALISED probabilities 2^(s - max) that feed the PV MFMAs (the row sum is taken over the unrounded p)
                                                      attention.hip:332-333,350 (version 1), :602-603,610 (version 2)
    - the output O / sum                              attention.hip:368 (version 1), :635 (version 2)
The largest distance between the two modes on the inputs of a case is the `d16` of that case: what the fp16 storage of a correct kernel costs.
"""
import numpy as np

HEAD_DIM = 64


def r16(x):
    """Round to the nearest fp16 (ties to even) and return as float64."""
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def visible(T, window):
    """[T, T] bool: visible[i, j] = key j is seen by query i."""
    wl, wr = window
    assert wl >= 0 and wr >= 0, "a finite window (left, right) is required"
    i = np.arange(T)[:, None]
    j = np.arange(T)[None, :]
    m = (j >= i - wl) & (j <= i + wr)
    assert m.any(axis=1).all()          # the diagonal is always inside a window with wl, wr >= 0: no query is left without a key
    return m


def attend_one(q, k, v, mask, base2=False, p16=None, out16=False):
    """One (chunk, head): q, k, v [T, d] float64, mask [T, T] -> [T, d]. p16: None | "normalised" | "unnormalised"."""
    s = q @ k.T
    s = np.where(mask, s, -np.inf)
    m = s.max(axis=1, keepdims=True)
    p = np.exp2(s - m) if base2 else np.exp(s - m)
    z = p.sum(axis=1, keepdims=True)
    if p16 == "normalised":
        o = r16(p / z) @ v
    elif p16 == "unnormalised":
        o = (r16(p) @ v) / z
    else:
        assert p16 is None
        o = (p @ v) / z
    return r16(o) if out16 else o


def windowed_attention(q, k, v, window, base2=False, p16=None, out16=False, pairs=None):
    """q, k, v [N, T, H, d] -> [N, T, H, d] float64. `pairs`: iterable of (chunk, head) to compute (the others stay NaN); None = all."""
    N, T, H, d = q.shape
    mask = visible(T, window)
    out = np.full((N, T, H, d), np.nan)
    for n, h in (pairs if pairs is not None else all_pairs(N, H)):
        qq, kk, vv = (np.asarray(a[n, :, h], np.float64) for a in (q, k, v))
        out[n, :, h] = attend_one(qq, kk, vv, mask, base2, p16, out16)
    return out


def all_pairs(N, H):
    return [(n, h) for n in range(N) for h in range(H)]


def brute_force(q, k, v, window, base2=False):
    """Triple loop over (query, key, feature) per (chunk, head), python floats: for tiny T only."""
    import math
    N, T, H, d = q.shape
    wl, wr = window
    out = np.zeros((N, T, H, d))
    for n in range(N):
        for h in range(H):
            for i in range(T):
                js = [j for j in range(T) if i - wl <= j <= i + wr]
                assert js, "a query without a visible key"
                sc = [sum(float(q[n, i, h, e]) * float(k[n, j, h, e]) for e in range(d)) for j in js]
                mx = max(sc)
                w = [(2.0 ** (x - mx)) if base2 else math.exp(x - mx) for x in sc]
                z = sum(w)
                for e in range(d):
                    out[n, i, h, e] = sum(wj * float(v[n, j, h, e]) for wj, j in zip(w, js)) / z
    return out


def rotary_angles(T, d=HEAD_DIM):
    """[T, d/2] float64: position * 10000^(-2i/d) (flash-attn convention, interleaved=False; oracle/nn_ref.py::rotary)."""
    inv = 1.0 / (10000.0 ** (np.arange(0, d, 2, dtype=np.float64) / d))
    return np.arange(T, dtype=np.float64)[:, None] * inv[None, :]


def rotate(x, inverse=False):
    """x [N, T, H, d] -> rotary embedding applied along T (inverse: rotated back)."""
    x = np.asarray(x, np.float64)
    N, T, H, d = x.shape
    ang = rotary_angles(T, d)
    cos, sin = np.cos(ang)[None, :, None, :], np.sin(ang)[None, :, None, :]
    if inverse:
        sin = -sin
    x1, x2 = x[..., :d // 2], x[..., d // 2:]
    return np.concatenate([x1 * cos - x2 * sin, x1 * sin + x2 * cos], axis=-1)


def pair_inputs(entry, qkv, n, h, storage_fp16=False):
    """(q, k, v) [T, 64] float64 of one (chunk, head) as the kernel of `entry` ("general" | "ring") multiplies them: packed qkv
    [N, T, 3, H, 64] holds the fp16 values the kernel is given."""
    q, k, v = (np.asarray(qkv[n:n + 1, :, i, h:h + 1], np.float64) for i in range(3))
    if entry == "general":
        q, k = rotate(q) * 0.125, rotate(k)
        if storage_fp16:
            q, k = r16(q), r16(k)
    else:
        assert entry == "ring"
    return q[0, :, 0], k[0, :, 0], v[0, :, 0]


def _entry(entry, qkv, window, storage_fp16, pairs):
    N, T, three, H, d = qkv.shape
    assert three == 3 and d == HEAD_DIM
    mask = visible(T, window)
    p16 = None if not storage_fp16 else "normalised" if entry == "general" else "unnormalised"
    out = np.full((N, T, H, d), np.nan)
    for n, h in (pairs if pairs is not None else all_pairs(N, H)):
        q, k, v = pair_inputs(entry, qkv, n, h, storage_fp16)
        out[n, :, h] = attend_one(q, k, v, mask, entry == "ring", p16, storage_fp16)
    return out.reshape(N, T, H * d)


def bh_attention(qkv, window, storage_fp16=False, pairs=None):
    """Packed qkv [N, T, 3, H, 64] (the fp16 values the kernel is given) -> [N, T, H*64] float64: rotary on q and k, scale 1/8, natural base.
    Pairs (chunk, head) not in `pairs` stay NaN."""
    return _entry("general", qkv, window, storage_fp16, pairs)


def bh_attention_prerotated(qkv, window, storage_fp16=False, pairs=None):
    """Packed qkv [N, T, 3, H, 64] with q, k already rotated and q scaled by log2(e) / 8 -> [N, T, H*64] float64: softmax in base 2."""
    return _entry("ring", qkv, window, storage_fp16, pairs)


def probe_effects(q, k, v, mask, jx, kx, vx, base2=False):
    """One (chunk, head), every query a probe of ONE key: how much does query i's fp64 output move (largest feature) when its probed key is
    taken out of the visible set (jx[i] >= 0: the visible key of that column) or put into it (jx[i] < 0: the key (kx[i], vx[i]) - one outside
    the window, one of a neighbouring chunk, or an all-zero staging row)? Removing the only visible key leaves the query without keys: the
    kernels write 0 then, so the effect is |output|. q, k, v, kx, vx [T, d], mask [T, T], jx [T] -> [T]"""
    T = q.shape[0]
    exp = np.exp2 if base2 else np.exp
    s = np.where(mask, q @ k.T, -np.inf)
    m = s.max(axis=1, keepdims=True)
    p = exp(s - m)
    z = p.sum(axis=1, keepdims=True)
    acc = p @ v
    o = acc / z
    # put in: the extra key's weight relative to the row's maximum may exceed 1 by far (a masked key with the largest raw score): fp64 holds it
    px = exp((q * kx).sum(axis=1, keepdims=True) - m)
    added = (acc + px * vx) / (z + px)
    # taken out: the softmax over the remaining keys, recomputed (no cancellation)
    rows = np.nonzero(jx >= 0)[0]
    assert mask[rows, jx[rows]].all(), "a probe that claims to be seen is not in the window"
    s2 = s.copy()
    s2[rows, jx[rows]] = -np.inf
    m2 = s2.max(axis=1, keepdims=True)
    alone = np.isneginf(m2)
    p2 = exp(s2 - np.where(alone, 0.0, m2))
    removed = np.where(alone, 0.0, (p2 @ v) / np.where(alone, 1.0, p2.sum(axis=1, keepdims=True)))
    o2 = np.where((jx >= 0)[:, None], removed, added)
    return np.abs(o2 - o).max(axis=1)


def key_effect(q_i, k_vis, v_vis, k_x, v_x, base2=False, remove=None):
    """Largest change of one query's fp64 output when ONE key is taken out of / put into its visible set.
    q_i [d]; k_vis, v_vis [n, d] the visible keys; remove = index into them to take out, or None to ADD the key (k_x, v_x)."""
    def out(kk, vv):
        s = kk @ q_i
        p = np.exp2(s - s.max()) if base2 else np.exp(s - s.max())
        return (p @ vv) / p.sum()
    base = out(k_vis, v_vis)
    if remove is not None:
        keep = np.arange(len(k_vis)) != remove
        assert keep.any(), "removing the only visible key"
        other = out(k_vis[keep], v_vis[keep])
    else:
        other = out(np.concatenate([k_vis, k_x[None]]), np.concatenate([v_vis, v_x[None]]))
    return float(np.abs(other - base).max())

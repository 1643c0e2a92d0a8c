"""Window-edge probes for the training attention backward (attn_bwd_q_kernel<NT> / attn_bwd_kv_kernel<NT>): the inputs, the case list and
the decisiveness figures of the sweep in tests/test_gpu_attention_train.py, checked without a device by
tests/test_attention_train_ref_cpu.py. Host only; builds on tests/attention_ref.py and tests/attention_train_ref.py; no import of bonito_amd.

WHY PROBES. On Gaussian inputs under a wide window one (query, key) pair moves dq_i, dk_j, dv_j by about one key's softmax weight, which
a max-norm over the tensor does not separate from 4 d16. Here every query is a probe whose gradients hang on ONE pair.

INPUTS (seeded). Keys are near-orthogonal unit vectors (+-1/8 per feature), rotated back so that the kernel's rotary reproduces them (the
construction of make_case("general", "edge", ...) in tests/test_gpu_attention.py); v is Gaussian. A one-hot query does not work in the
backward: with P_ij ~ 1, dS = P (dP - delta) ~ 0. So query i splits its mass between two keys, q_i = BETA (k_target + k_i) with BETA = 128:
both score about 16 after the 1/8 scale, every other key about +-3; and the upstream gradient is aimed at their difference,
dO_i = v_target - v_i, so that dP_i,target - dP_ii = |v_target - v_i|^2 ~ 128. The target cycles by (i + 2 n + 3 h) mod 5 over the offsets
    -wl, +wr          the key must be seen, in both passes: P ~ 1/2 on either key, dS ~ +-32
    -wl - 1, +wr + 1  the key must NOT be seen: P_ii ~ 1 and dS ~ 0, but P ~ 1, dS ~ 128 on the pair if it is let in
    0                 self only (Gaussian dO); so is any probe whose target is the query itself (wl = 0 or wr = 0)
SEAMS. The rows of all chunks are contiguous in memory. A target outside the chunk points at the row that occupies that memory position,
row (n T + target) mod T of chunk (n T + target) div T - the neighbouring chunk, or one further away where the chunks are shorter than the
window. That row must not be seen. Past either end of the batch there is no row, and the probe becomes self only.
ALL-ZERO STAGING ROWS need no probe: a staged row outside [0, T) that is let in contributes dS . 0 to dq (its k~ is 0) and P . 0 to dk and
dv (the key pass stages q~ = dO = 0 for it), in either pass; the forward's sweep owns the one place where a zero row matters (the softmax sum).

EFFECT of a wrong decision about the probed pair (query (n, i), key (m, r)), from the reference alone, with the forward's lse and out - and
so delta - unchanged, as the kernels would have them: P = exp(q~_i . k~_r - lse_i), dS = P (dO_i . v_r - delta_i), and
    flipped in the query pass only: dq_i moves by rot^-1_i(dS k~_r) / 8             (k~, v of the other row)
    flipped in the key pass only:   dk_r moves by rot^-1_r(dS q~_i), dv_r by P dO_i    (q~, dO, lse, delta of the other row)
each measured at its largest feature. `references` returns the smallest of each over all pair probes of a case.

CRITERION. Per case and part, max|kernel - exact| <= 4 d16 with d16 = max|exact(storage_fp16=True, fp32_places=True) - exact()| in absolute
terms, and in front of every launch 4 d16 < smallest effect / 10 (`check_decisive`). fp32_places: see attention_train_ref - probes that must
not be seen leave the exact dS at (almost) 0, where fp16 storage costs nothing and the kernels' two fp32 sums are all that is left.
"""
import numpy as np

import attention_ref as ar
import attention_train_ref as tr

BETA = 128.0
OFFSETS = 5                                   # -wl, +wr, -wl - 1, +wr + 1, 0
FACTOR = 4.0                                  # the project's factor for attention


def need_tiles(window):
    return (16 + window[0] + window[1] + 15) // 16          # tiles one wave can see -> <6 | 10 | 18 | 26> in either pass


def sweep_length(window):
    """The smallest T with one INTERIOR block of 128 whose staged rows all lie inside the chunk, in both passes: b blocks in front of it with
    128 b >= max(wl, wr), the block, and max(wl, wr) + 1 rows behind it."""
    w = max(window)
    return 128 * (-(-w // 128)) + 128 + w + 1


# (N, T, H, window, need)
RUNG_CASES = [                                 # every rung on both sides of its boundary; T = sweep_length + 0 .. 15, T % 16 != 0 in about half
    (1, 297, 2, (40, 40), 6),
    (1, 352, 1, (80, 0), 6),
    (2, 337, 1, (0, 80), 6),
    (1, 304, 2, (40, 41), 7),
    (1, 338, 1, (81, 0), 7),
    (1, 352, 1, (0, 81), 7),
    (1, 329, 2, (72, 72), 10),
    (1, 544, 1, (144, 0), 10),
    (1, 529, 1, (0, 144), 10),
    (1, 336, 2, (72, 73), 11),
    (1, 530, 1, (0, 145), 11),
    (1, 521, 2, (136, 136), 18),
    (1, 800, 1, (0, 272), 18),
    (1, 785, 1, (272, 0), 18),
    (1, 528, 2, (136, 137), 19),
    (1, 786, 1, (273, 0), 19),
    (1, 585, 2, (200, 200), 26),
    (1, 1056, 1, (400, 0), 26),
    (1, 1041, 1, (0, 400), 26),
]
EDGE_CASES = [                                 # T edges on a middle rung; N so that the window reaches rows of other chunks where T is short
    (90, 1, 1, (40, 41), 7),                   # T = 1: every row its own chunk, the window spans 81 of them
    (4, 17, 2, (40, 41), 7),
    (2, 127, 1, (40, 41), 7),
    (2, 128, 1, (40, 41), 7),
    (2, 129, 2, (40, 41), 7),                  # one row in the second block
    (1, 257, 1, (40, 41), 7),
    (280, 1, 1, (136, 137), 19),
    (10, 17, 1, (136, 137), 19),
    (3, 127, 1, (136, 137), 19),               # the window wider than the chunk
    (3, 128, 1, (136, 137), 19),
    (3, 129, 1, (136, 137), 19),
    (1, 257, 2, (136, 137), 19),
    (1, 130, 2, (0, 0), 1),                    # one visible key: exact dq = dk = 0
    (1, 130, 2, (1, 7), 2),
]
SEAM_CASES = [                                 # every chunk shorter than the window: seam probes dominate
    (3, 129, 2, (40, 41), 7),
    (3, 144, 2, (200, 200), 26),
    (3, 130, 3, (1, 7), 2),
]
CASES = RUNG_CASES + EDGE_CASES + SEAM_CASES
PLANE_CASES = [(1, 304, 2, (40, 41), 7), (3, 144, 2, (200, 200), 26)]          # the probe cases on which lse and delta are checked as well


def case_id(case):
    return str(tuple(case)).replace(" ", "")


def case_seed(case):
    N, T, H, (wl, wr), _ = case
    return N * 104729 + T * 31 + H + wl * 3 + wr


def make_probe_case(N, T, H, window, seed):
    """-> (qkv fp16 [N, T, 3, H, 64], dout fp16 [N, T, H*64], probes). probes: dict of [N, T, H] arrays - `pair` (bool: the query probes a
    pair; False: self only), `seen` (bool: the pair must be seen), `pn`, `pt` (chunk and row of the probed key; the query's own where not
    a pair)."""
    wl, wr = window
    rng = np.random.default_rng(seed)
    k = (rng.integers(0, 2, (N, T, H, 64)).astype(np.float64) * 2 - 1) / 8
    v = rng.standard_normal((N, T, H, 64)).astype(np.float16).astype(np.float64)
    n_i, t_i, h_i = np.meshgrid(np.arange(N), np.arange(T), np.arange(H), indexing="ij")
    kidx = (t_i + 2 * n_i + 3 * h_i) % OFFSETS
    off = np.array([-wl, wr, -wl - 1, wr + 1, 0])[kidx]
    flat = n_i * T + t_i + off                                # the memory position of the target row
    pair = (off != 0) & (flat >= 0) & (flat < N * T)
    pn = np.where(pair, flat // T, n_i)
    pt = np.where(pair, flat % T, t_i)
    seen = pair & (pn == n_i) & (kidx < 2)
    q = BETA * (k[pn, pt, h_i] + k)
    dout = np.where(pair[..., None], v[pn, pt, h_i] - v, rng.standard_normal((N, T, H, 64)))
    q, k = ar.rotate(q, inverse=True), ar.rotate(k, inverse=True)
    qkv = np.stack([q, k, v], axis=2).astype(np.float16)
    return qkv, dout.reshape(N, T, H * 64).astype(np.float16), {"pair": pair, "seen": seen, "pn": pn, "pt": pt}


def _unrotate(x, pos, T):
    """x [P, 64] rotated vectors at rows pos [P] of a chunk of T rows -> rotated back."""
    ang = ar.rotary_angles(T)[pos]
    cos, sin = np.cos(ang), -np.sin(ang)
    x1, x2 = x[:, :32], x[:, 32:]
    return np.concatenate([x1 * cos - x2 * sin, x1 * sin + x2 * cos], axis=1)


def probe_effects(qkv, dout, probes, lse, delta, reduce=np.min):
    """The module docstring's EFFECT for every pair probe -> {part: smallest over the probes} (None: the case has no pair probe).
    lse, delta [N, H, T]: the exact forward's (attention_train_ref.exact(..., stats=True)). `reduce`: another statistic than the smallest."""
    qkv = np.asarray(qkv, np.float64)
    N, T, _, H, d = qkv.shape
    do = np.asarray(dout, np.float64).reshape(N, T, H, d)
    qt, kt, v = ar.rotate(qkv[:, :, 0]) * 0.125, ar.rotate(qkv[:, :, 1]), qkv[:, :, 2]
    n, t, h = np.nonzero(probes["pair"])
    if len(n) == 0:
        return None
    m, r = probes["pn"][n, t, h], probes["pt"][n, t, h]
    s = (qt[n, t, h] * kt[m, r, h]).sum(axis=1)                 # one formula for a pair that is seen and one that is not
    p = np.exp(s - lse[n, h, t])
    ds = p * ((do[n, t, h] * v[m, r, h]).sum(axis=1) - delta[n, h, t])
    eq = np.abs(_unrotate(ds[:, None] * kt[m, r, h], t, T)).max(axis=1) * 0.125
    ek = np.abs(_unrotate(ds[:, None] * qt[n, t, h], r, T)).max(axis=1)
    ev = np.abs(p[:, None] * do[n, t, h]).max(axis=1)
    return {"dq": float(reduce(eq)), "dk": float(reduce(ek)), "dv": float(reduce(ev))}


def references(case):
    """-> dict of a case, from the references alone: qkv, dout, probes; want = (out, dq, dk, dv, lse, delta) exact in fp64; d16 = {dq, dk, dv,
    lse: max|exact with fp16 storage - exact|}; effects = {dq, dk, dv: smallest probe effect}."""
    N, T, H, window, need = case
    assert need_tiles(window) == need, case
    qkv, dout, probes = make_probe_case(N, T, H, window, case_seed(case))
    want = tr.exact(qkv, dout, window, stats=True)
    got = tr.exact(qkv, dout, window, storage_fp16=True, fp32_places=True, stats=True)
    d16 = {name: float(np.abs(g - w).max()) for name, g, w in zip(tr.PARTS + ("lse",), got[1:5], want[1:5])}
    return {"qkv": qkv, "dout": dout, "probes": probes, "want": want, "d16": d16,
            "effects": probe_effects(qkv, dout, probes, want[4], want[5])}


def check_decisive(name, d16, effects):
    """4 d16 lies below a tenth of the smallest probe effect, per part: the tolerance cannot hide a wrong decision about one pair."""
    assert effects is not None, "%s: no pair probe" % name
    for part in tr.PARTS:
        assert FACTOR * d16[part] < effects[part] / 10, "%s %s: tolerance 4 x d16 = %.3e is not below a tenth of the smallest probe effect %.3e" % (
            name, part, FACTOR * d16[part], effects[part])


def errors(got, want):
    """{part: max|got - want|} over dq, dk, dv; got = (dq, dk, dv), want = exact's result. A non-finite element is inf."""
    out = {}
    for name, g, w in zip(tr.PARTS, got, want[1:4]):
        g = np.asarray(g, np.float64)
        out[name] = float(np.abs(g - w).max()) if np.isfinite(g).all() else float("inf")
    return out

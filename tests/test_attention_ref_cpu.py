"""Pins tests/attention_ref.py (the fp64 reference of tests/test_gpu_attention.py) on the host: equal to the SDPA formulation of
oracle/nn_ref.py (`rotary` + `window_mask` + softmax, which the tf_*.npz reference fixtures pin) to fp32 rounding, equal to a triple-loop
brute force at small T, and no query is ever left without a visible key."""
import numpy as np
import pytest
import torch

import attention_ref as ar
from oracle import nn_ref

LOG2E = 1.4426950408889634


def _qkv(N, T, H, seed, scale=0.8):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, T, 3, H, 64, generator=g) * scale).half()


def _sdpa_fp32(qkv, win):
    """tests/test_gpu_ops.py::test_attention_matches_sdpa_restatement's `want`, in fp32."""
    N, T, _, H, d = qkv.shape
    r = nn_ref.rotary(qkv.float())
    q, k, v = (r[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    s = (q @ k.transpose(-1, -2)) / 8.0
    s = s.masked_fill(~nn_ref.window_mask(T, win), float("-inf"))
    return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(N, T, H * d).numpy().astype(np.float64)


@pytest.mark.parametrize("N,T,H,win", [(2, 100, 2, (31, 32)), (1, 300, 1, (127, 128)), (2, 50, 3, (5, 0)), (1, 130, 2, (0, 7)),
                                       (1, 64, 1, (200, 200)), (1, 1, 1, (0, 0)), (1, 17, 2, (0, 144))])
def test_equals_the_oracle_sdpa_formulation_to_fp32_rounding(N, T, H, win):
    qkv = _qkv(N, T, H, T + H)
    want = _sdpa_fp32(qkv, win)
    got = ar.bh_attention(qkv.numpy(), win)
    # fp32 evaluation of sums of <= 64 (scores) and <= T (P V) products of O(1) terms: 1e-5 is ~100 fp32 spacings of the outputs
    assert np.abs(got - want).max() < 1e-5
    # the pre-rotated convention on the same problem: q, k rotated (and q scaled by log2(e) / 8) by the caller, softmax in base 2
    x = qkv.numpy().astype(np.float64)
    pre = np.stack([ar.rotate(x[:, :, 0]) * (0.125 * LOG2E), ar.rotate(x[:, :, 1]), x[:, :, 2]], axis=2)
    assert np.abs(ar.bh_attention_prerotated(pre, win) - got).max() < 1e-12


@pytest.mark.parametrize("T,win", [(1, (0, 0)), (5, (0, 0)), (12, (3, 2)), (12, (0, 4)), (11, (4, 0)), (7, (100, 100)), (12, (1, 11))])
@pytest.mark.parametrize("base2", [False, True])
def test_equals_a_triple_loop_brute_force(T, win, base2):
    rng = np.random.default_rng(T * 31 + win[0] * 7 + win[1])
    q, k, v = (rng.standard_normal((2, T, 2, 8)) for _ in range(3))
    got = ar.windowed_attention(q, k, v, win, base2=base2)
    assert np.abs(got - ar.brute_force(q, k, v, win, base2=base2)).max() < 1e-13


def test_rotary_matches_the_oracle_and_inverts():
    qkv = _qkv(1, 40, 2, 3)
    want = nn_ref.rotary(qkv.float()).numpy()
    x = qkv.numpy().astype(np.float64)
    for i in (0, 1):
        got = ar.rotate(x[:, :, i])
        assert np.abs(got - want[:, :, i]).max() < 2e-5          # fp32 angles of positions < 40
        assert np.abs(ar.rotate(got, inverse=True) - x[:, :, i]).max() < 1e-13


@pytest.mark.parametrize("T", [1, 2, 16, 300])
@pytest.mark.parametrize("win", [(0, 0), (0, 5), (5, 0), (128, 144), (1000, 1000)])
def test_no_query_is_left_without_a_visible_key(T, win):
    m = ar.visible(T, win)
    assert m.any(axis=1).all() and m[np.arange(T), np.arange(T)].all()
    assert m.sum() == sum(min(i + win[1], T - 1) - max(i - win[0], 0) + 1 for i in range(T))
    with pytest.raises(AssertionError):
        ar.visible(T, (-1, 0))


def test_storage_fp16_modes_round_where_documented():
    """The fp16 mode differs from fp64 by fp16-sized amounts only, its output is fp16-representable, and the two kernels' conventions differ
    (normalised against un-normalised probabilities): on a row whose softmax is spread over many keys the un-normalised p stay near 1 while
    the normalised ones are rounded at 1/n."""
    qkv = _qkv(1, 200, 1, 9, scale=0.7).numpy().astype(np.float64)
    for fn in (ar.bh_attention, ar.bh_attention_prerotated):
        a, b = fn(qkv, (40, 17)), fn(qkv, (40, 17), storage_fp16=True)
        d = np.abs(a - b).max()
        assert 0 < d < 2e-3 and np.array_equal(b, ar.r16(b))
    pairs = [(0, 0)]
    part = ar.bh_attention_prerotated(np.repeat(qkv, 2, axis=0), (40, 17), pairs=pairs)
    assert np.isnan(part[1]).all() and np.array_equal(part[0], ar.bh_attention_prerotated(qkv, (40, 17))[0])


def test_key_effect_is_the_output_change_of_one_key():
    rng = np.random.default_rng(5)
    k, v = rng.standard_normal((6, 8)), rng.standard_normal((6, 8))
    q = 3.0 * k[2]
    full = ar.attend_one(q[None], k, v, np.ones((1, 6), bool))[0]
    less = ar.attend_one(q[None], k[np.arange(6) != 2], v[np.arange(6) != 2], np.ones((1, 5), bool))[0]
    assert abs(ar.key_effect(q, k, v, None, None, remove=2) - np.abs(full - less).max()) < 1e-14
    assert abs(ar.key_effect(q, k[:5], v[:5], k[5], v[5]) - np.abs(
        ar.attend_one(q[None], k[:5], v[:5], np.ones((1, 5), bool))[0] - full).max()) < 1e-14


@pytest.mark.parametrize("base2", [False, True])
def test_probe_effects_equals_key_effect_row_by_row(base2):
    """The vectorised probe effect (every query takes one key out or lets one in) against the one-query statement, including a query whose
    only visible key is taken out (the kernels write 0 there: the effect is |output|)."""
    rng = np.random.default_rng(11)
    T, d, win = 9, 8, (2, 1)
    q, k, v = (rng.standard_normal((T, d)) for _ in range(3))
    mask = ar.visible(T, win)
    jx = np.array([0, -1, 1, -1, 5, -1, 6, -1, 8])                       # seen probes name a visible column
    kx, vx = rng.standard_normal((T, d)) * 3, rng.standard_normal((T, d))
    got = ar.probe_effects(q, k, v, mask, jx, kx, vx, base2=base2)
    for i in range(T):
        cols = np.nonzero(mask[i])[0]
        want = ar.key_effect(q[i], k[cols], v[cols], kx[i], vx[i], base2=base2,
                             remove=int(np.nonzero(cols == jx[i])[0][0]) if jx[i] >= 0 else None)
        assert abs(got[i] - want) < 1e-12, i
    alone = ar.probe_effects(q, k, v, ar.visible(T, (0, 0)), np.arange(T), kx, vx, base2=base2)
    assert np.abs(alone - np.abs(v).max(axis=1)).max() < 1e-15


def test_probe_cases_of_the_device_sweeps_are_decisive():
    """The condition the device tests assert, evaluated here from the reference alone on a few of their cases: 4 x d16 lies below a tenth
    of the smallest change that taking out / letting in the probed key makes."""
    import test_gpu_attention as tg
    for entry, kind, N, T, H, win in [("ring", "edge", 1, 193, 2, (0, 144)), ("ring", "edge", 2, 17, 1, (128, 128)),
                                      ("ring", "seam", 5, 33, 2, (127, 128)), ("general", "edge", 1, 291, 1, (0, 81)),
                                      ("general", "edge", 1, 1, 1, (0, 0))]:
        qkv, probes = tg.make_case(entry, kind, N, T, H, win, seed=T)
        ref, d16, smallest = tg.reference(entry, qkv, win, probes, ar.all_pairs(N, H))
        assert np.isfinite(ref).all() and smallest is not None and probes["probe"].any()
        tg.check_decisive("%s %s %s" % (entry, kind, win), d16, smallest)
        assert 4 * d16 < smallest / 10

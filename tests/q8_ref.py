"""The checker of the 8-bit recurrent path Q8-1 (csrc/lstm_q8.hip, defined in oracle/lstm_q8_ref.py): the reference side of
tests/test_gpu_q8.py, pinned by tests/test_q8_ref_cpu.py. numpy only; no import of bonito_amd.

Layout. A layer hands its int8 output on in MFMA B-fragment order [T][N/16 rings][ceil(H/64) k-steps][64 lanes][16 bytes]; unit u of
chunk c of a ring lives at byte `frag_byte(u, c)` of the ring's tile. Where H % 64 != 0 the last k-step has 64 - H % 64 PADDING units per
chunk that no kernel writes. `unscramble` returns the real units and the padding bytes apart, `scramble` is its inverse.

Check (`check_layer`), teacher forced, one step at a time, from what the kernel itself published:
  * x sums [T][N][4H] == quantise_act(x, bound) @ quantise_rows(w_ih)^T                       exactly
  * h sums of step t   == (the kernel's own int8 h of the step before) @ quantise_rows(w_hh)^T  exactly (zero at the first step)
  * hq[t] == rint(127 * h16[t]) and never -128                                                exactly
  * h16[t] against the cell evaluated in fp64 on the fp32 pre-activation the definition forms from those exact sums,
        pre = (float(sx_sum) * (s_ih * float(bound / 127)) + b) + float(sh_sum) * (s_hh / 127)     each operation rounded to fp32,
    with the cell state carried in fp64 from those same steps. The worst |h16 - h| is RETURNED; the caller holds it against its bound.
The integer products are taken in float64 (|sum| <= 512 * 127 * 127 < 2^53: exact) because numpy has no fast integer matmul.
A failed exact check raises AssertionError naming the step.

`saturating_case` is the data of the saturation test: biases of +-30 in eight sign patterns by unit (u % 8) so that i, f, g, o sit
beyond the +-25 / +-12.5 clamps of lstm_cell in both signs (pattern 0 lets c climb by one per step and drives h to +1, pattern 1 to -1),
weight rows that are all zero (scale 1.0), and inputs at +-10 * bound and +-65504.
"""
import numpy as np

from oracle import lstm_q8_ref

# the widths with a kernel instance (BH_LSTM_Q8_INSTANCES of csrc/lstm_q8.hip), and every row of that list as (H, variant) -> <NK8, MT, WPS>
SERVED = (64, 96, 128, 144, 192, 256, 288, 336, 384, 512)
INSTANCES = {(384, 0): (6, 3, 1), (384, 2): (6, 3, 2), (384, 1): (6, 1, 3), (96, 0): (2, 3, 1), (144, 0): (3, 3, 1), (288, 0): (5, 3, 1),
             (64, 0): (1, 4, 1), (128, 0): (2, 4, 1), (256, 0): (4, 4, 1), (512, 0): (8, 4, 1),
             (336, 0): (6, 3, 1), (192, 0): (3, 3, 1)}          # the second widths of (6,3,1) and (3,3,1)
SENTINEL = -128
SAT_SIGNS = ((1, 1, 1, 1), (1, 1, -1, 1), (-1, -1, -1, -1), (1, -1, 1, 1), (-1, 1, 1, 1), (1, 1, 1, -1), (0, 0, 0, 0), (1, -1, -1, 1))


def nk8(H):
    return (H + 63) // 64


def frag_byte(u, c):
    """Byte of unit u of chunk c (0..15) inside a ring tile: frag_byte<1>() of csrc/lstm_ring.h."""
    return ((((u >> 6) * 64 + ((u >> 4) & 3) * 16 + c) << 4) + (u & 15))


def unscramble(frag, T, N, H):
    """int8 fragment order (flat) -> (units [T][N][H], padding [T][N][64 * nk8 - H])."""
    k = nk8(H)
    a = np.asarray(frag).reshape(T, N // 16, k, 4, 16, 16)          # t, ring, ks, q, c, j
    a = a.transpose(0, 1, 4, 2, 3, 5).reshape(T, N, k * 64)
    return a[:, :, :H], a[:, :, H:]


def scramble(units, pad=None, fill=SENTINEL):
    """(units [T][N][H], padding [T][N][64 * nk8 - H] or a fill byte) -> flat int8 in fragment order."""
    T, N, H = units.shape
    k = nk8(H)
    if pad is None:
        pad = np.full((T, N, k * 64 - H), fill, np.int8)
    a = np.concatenate((units, pad), axis=2).reshape(T, N // 16, 16, k, 4, 16)       # t, ring, c, ks, q, j
    return np.ascontiguousarray(a.transpose(0, 1, 3, 4, 2, 5)).reshape(-1).astype(np.int8)


def check_fragments(frag, T, N, H, fill=SENTINEL):
    """A tile pre-filled with `fill` (0x80) after a layer wrote it: every real unit written (no fill byte left; -128 is no quantised
    value), every padding byte untouched. -> units [T][N][H]."""
    units, pad = unscramble(frag, T, N, H)
    assert not (units == fill).any(), "real units left unwritten or equal to the sentinel: %d" % int((units == fill).sum())
    assert (pad == fill).all(), "padding bytes written: %d" % int((pad != fill).sum())
    return units


def expected_x_sums(x, w_ih, bound):
    """-> (xq int8 [T][N][H], exact sums float64 [T][N][4H])."""
    q_ih, _ = lstm_q8_ref.quantise_rows(w_ih)
    xq = lstm_q8_ref.quantise_act(np.asarray(x, np.float32), bound)
    T, N, H = xq.shape
    return xq, (xq.reshape(T * N, H).astype(np.float64) @ q_ih.astype(np.float64).T).reshape(T, N, -1)


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def check_layer(x, w_ih, w_hh, bias, bound, reverse, h16, hq, sums):
    """x fp16/fp32 [T][N][H]; weights fp32 [4H][H]; bias fp32 [4H]; the kernel's h16 [T][N][H] fp16, hq [T][N][H] int8 (unscrambled),
    sums int32 [T][N][4H][2]. Raises on any exact mismatch; -> the worst |h16 - fp64 cell| over all steps."""
    x = np.asarray(x, np.float32)
    T, N, H = x.shape
    assert h16.shape == (T, N, H) and hq.shape == (T, N, H) and sums.shape == (T, N, 4 * H, 2)
    _, want_x = expected_x_sums(x, w_ih, bound)
    bad = sums[..., 0] != want_x
    assert not bad.any(), "x sums differ at %d places, first (t, n, row) = %s" % (int(bad.sum()), tuple(int(v[0]) for v in np.nonzero(bad)))
    _, s_ih = lstm_q8_ref.quantise_rows(w_ih)
    q_hh, s_hh = lstm_q8_ref.quantise_rows(w_hh)
    qh = q_hh.astype(np.float64).T
    sxs = s_ih * np.float32(bound / 127.0)
    shs = s_hh / np.float32(127.0)
    b = np.zeros(4 * H, np.float32) if bias is None else np.asarray(bias, np.float32)
    prev = np.zeros((N, H), np.float64)
    c = np.zeros((N, H), np.float64)
    worst = 0.0
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        bad = sums[t, :, :, 1] != prev @ qh
        assert not bad.any(), "h sums of step t = %d differ at %d places, first (n, row) = %s" % (
            t, int(bad.sum()), tuple(int(v[0]) for v in np.nonzero(bad)))
        pre = (sums[t, :, :, 0].astype(np.float32) * sxs + b) + sums[t, :, :, 1].astype(np.float32) * shs       # fp32, rounded per operation
        assert pre.dtype == np.float32
        i, f, g, o = np.split(pre.astype(np.float64), 4, axis=-1)
        c = _sig(f) * c + _sig(i) * np.tanh(g)
        h = _sig(o) * np.tanh(c)
        got = h16[t].astype(np.float64)
        assert np.isfinite(got).all(), "h16 of step t = %d is not finite" % t
        worst = max(worst, float(np.abs(got - h).max()))
        want_q = np.rint(h16[t].astype(np.float32) * np.float32(127.0))
        assert np.array_equal(hq[t], want_q), "hq != rint(127 h16) at step t = %d (%d places)" % (t, int((hq[t] != want_q).sum()))
        assert not (hq[t] == SENTINEL).any(), "hq holds the sentinel at step t = %d" % t
        prev = hq[t].astype(np.float64)
    return worst


def typical_case(H, T, N, bound=1.0, seed=0):
    """The data of the existing kernel-level test: rows of N(0,1) scaled by 0.02..0.12, bias N(0, 0.3), x ~ 0.6 bound N(0,1) clipped
    at 1.2 bound (a fifth of the inputs saturate the static scale). -> x fp16, w_ih, w_hh, bias fp32."""
    rng = np.random.default_rng(1000 * seed + H)
    w_ih = (rng.standard_normal((4 * H, H)) * rng.uniform(0.02, 0.12, (4 * H, 1))).astype(np.float32)
    w_hh = (rng.standard_normal((4 * H, H)) * rng.uniform(0.02, 0.12, (4 * H, 1))).astype(np.float32)
    bias = (rng.standard_normal(4 * H) * 0.3).astype(np.float32)
    x = np.clip(rng.standard_normal((T, N, H)) * 0.6 * bound, -1.2 * bound, 1.2 * bound).astype(np.float16)
    return x, w_ih, w_hh, bias


# units (by u % 16) whose four gate rows are all zero in w_ih and w_hh / in w_hh only
ZERO_BOTH, ZERO_HH = 6, 14


def saturating_case(H, T, N, bound=1.0, seed=0):
    """-> x fp16, w_ih, w_hh, bias fp32, and the positions (boolean [T][N][H]) of the inputs planted far beyond `bound`."""
    x, w_ih, w_hh, bias = typical_case(H, T, N, bound, seed + 17)
    unit = np.arange(H)
    signs = np.array(SAT_SIGNS, np.float32)[unit % 8]                 # [H][4]
    b4 = bias.reshape(4, H)
    sat = 30.0 * signs.T
    b4[...] = np.where(sat != 0, sat, b4)
    for gate in range(4):
        w_ih[gate * H + unit[unit % 16 == ZERO_BOTH]] = 0.0
        w_hh[gate * H + unit[unit % 16 == ZERO_BOTH]] = 0.0
        w_hh[gate * H + unit[unit % 16 == ZERO_HH]] = 0.0
    rng = np.random.default_rng(seed + 5)
    far = rng.random((T, N, H)) < 0.03
    vals = np.array([10.0 * bound, -10.0 * bound, 65504.0, -65504.0], np.float32)
    x = np.where(far, vals[rng.integers(0, 4, (T, N, H))], x.astype(np.float32)).astype(np.float16)
    return x, w_ih, w_hh, bias, far

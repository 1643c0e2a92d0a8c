"""tests/q8_ref.py pinned on the CPU (no GPU): the checker accepts the output of the definition itself
(oracle.lstm_q8_ref.lstm_q8_forward, integer sums recomputed in numpy, int8 h scrambled to fragment order and back) at the four widths
with the four last-k-step shapes (H % 64 = 0, 32, 16, 16), and rejects six planted errors; scramble / unscramble are the formula of
frag_byte() at every served width; and the host-side predicate q8_covers agrees with the launch plan on the served set."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import q8_ref
from oracle import lstm_q8_ref

T, N = 7, 32
TOL = 2e-3          # the project's bound on the cell (tests/test_gpu_q8.py)


def _module(w_ih, w_hh, bias, reverse):
    H = w_hh.shape[1]
    rnn = torch.nn.LSTM(H, H)
    with torch.no_grad():
        rnn.weight_ih_l0.copy_(torch.from_numpy(w_ih))
        rnn.weight_hh_l0.copy_(torch.from_numpy(w_hh))
        rnn.bias_ih_l0.copy_(torch.from_numpy(bias))
        rnn.bias_hh_l0.zero_()
    return types.SimpleNamespace(rnn=rnn, reverse=bool(reverse))


def emulate(case, bound, reverse, defect=None):
    """What a kernel publishes: (h16 fp16 [T][N][H], hq int8 [T][N][H], sums int32 [T][N][4H][2]). Without a defect, h16 is
    lstm_q8_forward's output and the sums are numpy integer products of the oracle's quantised operands."""
    x, w_ih, w_hh, bias = case
    H = x.shape[2]
    q_ih, s_ih = lstm_q8_ref.quantise_rows(w_ih)
    q_hh, s_hh = lstm_q8_ref.quantise_rows(w_hh)
    b = bias
    xq = lstm_q8_ref.quantise_act(x.astype(np.float32), bound).astype(np.int64)
    sx = (xq.reshape(T * N, H) @ q_ih.astype(np.int64).T).reshape(T, N, 4 * H)
    gx = sx.astype(np.float32) * (s_ih * np.float32(bound / 127.0)) + b
    run_rev = reverse and defect != "forwards"
    h16 = np.zeros((T, N, H), np.float16)
    hq = np.zeros((T, N, H), np.int8)
    sums = np.zeros((T, N, 4 * H, 2), np.int32)
    prev = np.zeros((N, H), np.int64)
    c = np.zeros((N, H), np.float32)
    for s in range(T):
        t = T - 1 - s if run_rev else s
        hin = prev
        if defect == "ring_neighbour" and s == 3:
            hin = prev.copy()
            hin[16:32] = prev[0:16]
        sh = hin @ q_hh.astype(np.int64).T
        g = gx[t] + sh.astype(np.float32) * (s_hh / np.float32(127.0))
        i, f, gg, o = np.split(g, 4, axis=-1)
        if defect == "swap_if":             # unit 5: the cell takes gate i for f and f for i; the sums are the right ones
            i, f = i.copy(), f.copy()
            i[:, 5], f[:, 5] = f[:, 5].copy(), i[:, 5].copy()
        c = (lstm_q8_ref._sigmoid(f) * c + lstm_q8_ref._sigmoid(i) * np.tanh(gg)).astype(np.float32)
        h = (lstm_q8_ref._sigmoid(o) * np.tanh(c)).astype(np.float32)
        h16[t] = h.astype(np.float16)
        hq[t] = lstm_q8_ref.quantise_act(h16[t].astype(np.float32), 1.0)
        sums[t, :, :, 0] = sx[t]
        sums[t, :, :, 1] = sh
        prev = hq[t].astype(np.int64)
    if defect == "slice_swap":              # chunk 3 at t = 2: the units of slice 1 and slice 2 (U = 12 / 16 units each) change places
        U = 4 * q8_ref.INSTANCES[(H, 0)][1]
        for a in (h16, hq):
            a[2, 3, U:2 * U], a[2, 3, 2 * U:3 * U] = a[2, 3, 2 * U:3 * U].copy(), a[2, 3, U:2 * U].copy()
    if defect == "hq_off_by_one":
        hq[4, 17, H - 1] += 1 if hq[4, 17, H - 1] < 127 else -1
    return h16, hq, sums


def _check(case, bound, reverse, got):
    x, w_ih, w_hh, bias = case
    h16, hq, sums = got
    frag = q8_ref.scramble(hq)
    units = q8_ref.check_fragments(frag, T, N, x.shape[2])
    return q8_ref.check_layer(x, w_ih, w_hh, bias, bound, reverse, h16, units, sums)


@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("H", [64, 96, 144, 336])
def test_checker_accepts_the_definition(H, reverse):
    bound = 3.5 if H == 144 else 1.0
    case = q8_ref.typical_case(H, T, N, bound, seed=1)
    got = emulate(case, bound, reverse)
    with torch.no_grad():
        want = lstm_q8_ref.lstm_q8_forward(_module(*case[1:], reverse), torch.from_numpy(case[0].astype(np.float32)), bound).numpy()
    assert np.array_equal(got[0].astype(np.float32), want)          # the emulation IS the definition
    worst = _check(case, bound, reverse, got)
    print("H %d reverse %d: worst cell error %.3g" % (H, reverse, worst))
    assert worst < 2.0 ** -11          # the definition differs from the fp64 cell by the fp16 rounding of h (half an ulp, |h| < 1) + fp32 noise


@pytest.mark.parametrize("defect", ["hq_off_by_one", "slice_swap", "ring_neighbour", "swap_if", "forwards"])
@pytest.mark.parametrize("H", [96, 144])
def test_checker_rejects_a_planted_error(H, defect):
    reverse = 1 if defect == "forwards" else 0
    case = q8_ref.typical_case(H, T, N, 1.0, seed=2)
    if defect == "swap_if":          # make i and f of the unit differ by far more than the tolerance
        case[3][5], case[3][H + 5] = 3.0, -3.0
    got = emulate(case, 1.0, reverse, defect)
    try:
        worst = _check(case, 1.0, reverse, got)
    except AssertionError as e:
        print("%s: %s" % (defect, e))
        assert defect != "swap_if"          # the sums of that run are right: it must fall to the cell tolerance
        return
    print("%s: worst cell error %.3g" % (defect, worst))
    assert defect == "swap_if" and worst >= TOL, (defect, worst)


@pytest.mark.parametrize("H", [144, 336, 96])
def test_checker_rejects_a_padding_byte_counted_as_a_unit(H):
    """A producer that puts unit H - 1 one place further (the first padding unit of the chunk), or a quantiser that leaves the sentinel
    in a real unit."""
    rng = np.random.default_rng(H)
    units = rng.integers(-127, 128, (T, N, H)).astype(np.int8)
    frag = q8_ref.scramble(units)
    assert np.array_equal(q8_ref.check_fragments(frag, T, N, H), units)
    bad = frag.copy()
    tile = q8_ref.nk8(H) * 1024
    at = (3 * (N // 16) + 1) * tile          # t = 3, ring 1
    bad[at + q8_ref.frag_byte(H, 9)] = bad[at + q8_ref.frag_byte(H - 1, 9)]
    bad[at + q8_ref.frag_byte(H - 1, 9)] = q8_ref.SENTINEL
    with pytest.raises(AssertionError):
        q8_ref.check_fragments(bad, T, N, H)
    only_pad = frag.copy()
    only_pad[at + q8_ref.frag_byte(64 * q8_ref.nk8(H) - 1, 15)] = 0
    with pytest.raises(AssertionError, match="padding"):
        q8_ref.check_fragments(only_pad, T, N, H)


@pytest.mark.parametrize("H", q8_ref.SERVED)
def test_scramble_is_frag_byte(H):
    k = q8_ref.nk8(H)
    tile = k * 1024
    t_n, n_n = 2, 32
    units = (np.arange(t_n * n_n * H) % 251 - 125).astype(np.int8).reshape(t_n, n_n, H)
    pad = (np.arange(t_n * n_n * (64 * k - H)) % 7 + 1).astype(np.int8).reshape(t_n, n_n, 64 * k - H)
    frag = q8_ref.scramble(units, pad)
    assert frag.shape == (t_n * (n_n // 16) * tile,)
    u, c = np.meshgrid(np.arange(64 * k), np.arange(16), indexing="ij")
    off = q8_ref.frag_byte(u, c)                                   # [unit][chunk]
    assert sorted(off.reshape(-1).tolist()) == list(range(tile))  # a bijection onto the tile
    full = np.concatenate((units, pad), axis=2)
    for t in range(t_n):
        for ring in range(n_n // 16):
            got = frag[(t * (n_n // 16) + ring) * tile:][off]      # [unit][chunk]
            assert np.array_equal(got.T, full[t, ring * 16:ring * 16 + 16])
    back_u, back_p = q8_ref.unscramble(frag, t_n, n_n, H)
    assert np.array_equal(back_u, units) and np.array_equal(back_p, pad)


def test_saturating_case_has_what_it_promises():
    H = 96
    x, w_ih, w_hh, bias, far = q8_ref.saturating_case(H, 9, 16, 3.5)
    b4 = bias.reshape(4, H)
    for gate in range(4):
        assert (b4[gate] == 30.0).any() and (b4[gate] == -30.0).any()
    rows = np.arange(4 * H)
    assert (np.abs(w_ih).max(axis=1) == 0).sum() == 4 * (H // 16) and (np.abs(w_hh).max(axis=1) == 0).sum() == 8 * (H // 16)
    assert lstm_q8_ref.quantise_rows(w_ih)[1][rows[np.abs(w_ih).max(axis=1) == 0]].tolist() == [1.0] * (4 * (H // 16))
    xf = x.astype(np.float32)
    assert far.any() and set(np.unique(xf[far]).tolist()) == {-65504.0, -35.0, 35.0, 65504.0}
    assert np.isfinite(xf).all() and (np.abs(lstm_q8_ref.quantise_act(xf, 3.5)[far]) == 127).all()


def test_served_set_is_the_launch_plan_and_q8_covers():
    from bonito_amd import _lib
    from bonito_amd.crf.basecall import q8_covers
    handle = _lib.lib()
    served = []
    for H in range(16, 1025, 16):
        out = (C.c_int32 * 17)()
        rc = handle.bh_lstm_launch_plan(_lib.LSTM_FAMILIES["q8"], H, 0, 1, 256, out, 17)
        has = out[0] == 1
        assert (rc == 0) == has, (H, rc, _lib.last_error())
        assert q8_covers(H) == has, H
        if has:
            served.append(H)
            assert tuple(out[14:17]) == q8_ref.INSTANCES[(H, 0)], H
    assert tuple(served) == q8_ref.SERVED == (64, 96, 128, 144, 192, 256, 288, 336, 384, 512)
    for variant in (1, 2):
        out = (C.c_int32 * 17)()
        assert handle.bh_lstm_launch_plan(_lib.LSTM_FAMILIES["q8"], 384, variant, 1, 256, out, 17) == 0
        assert tuple(out[14:17]) == q8_ref.INSTANCES[(384, variant)]
    assert len(set(q8_ref.INSTANCES.values())) == 10          # every row of BH_LSTM_Q8_INSTANCES

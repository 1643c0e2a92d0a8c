"""The 8-bit recurrent path Q8-1 on the GPU (-m gpu): `lstm_layer_q8_kernel` against its definition, oracle/lstm_q8_ref.py.

* the integer part is checked EXACTLY: the int32 sums the kernel's gate arithmetic starts from (test hook of
  bh_lstm_q8_layer) equal numpy's integer matmuls of the oracle's quantised weights with the quantised input / with the int8
  h the kernel itself published one step earlier; the published int8 h is rint(127 * fp16 h);
* the cell (fast exp / rcp on the GPU, libm on the CPU) is checked on those exact pre-activations within 2e-3;
* end to end, the engine with quantize=True stays within the oracle's stated bound of the fp32 oracle and decodes the same
  Viterbi paths on hac- and fast-shaped synthetic models.
koi's own int8 kernels are closed source: parity with koi is unpinned; Q8-1 is this repository's definition.

The checker lives in tests/q8_ref.py (pinned by tests/test_q8_ref_cpu.py). The hook bh_lstm_q8_layer launches one of three instances
of lstm_layer_q8_kernel<NK8, MT, WPS, LAST, DBG>, chosen by the outputs it is given, as forward_lstm_q8 chooses:
    mode "dbg"    sums given                  <.., true,  true >   tests only: dumps the int32 sums, forms xpre late
    mode "last"   h16_out, no sums            <.., true,  false>   the product's last recurrent layer
    mode "inner"  hq_frag only, no h16_out    <.., false, false>   the product's layers before it: int8 fragments only
What the kernel-level tests launch, each row in all three modes (x = both directions):
    H    variant  <NK8, MT, WPS>   every_instance (N 32, T 11)   short (N 16, T 1..6, 9)   forced split (N 48)   saturation (N 16, T 9)
    64   0        <1, 4, 1>        x                             x                         x
    96   0        <2, 3, 1>        x                                                       x                     x
    128  0        <2, 4, 1>        x                                                       x
    144  0        <3, 3, 1>        x                                                       x
    192  0        <3, 3, 1>        x                                                       x
    256  0        <4, 4, 1>        x                                                       x
    288  0        <5, 3, 1>        x                                                       x
    336  0        <6, 3, 1>        x                             x                         x
    384  0        <6, 3, 1>        x                             x                         x                     x
    384  1        <6, 1, 3>        x
    384  2        <6, 3, 2>        x
    512  0        <8, 4, 1>        x                                                       x
(the forced split, through bh_lstm_q8_layer_split, runs "dbg" at 1, 2 and all rings per launch, "last" at 1 and "inner" at 2). H = 384 variant 0
also runs one ring past the device's own launch size ("dbg" and "last"). The three modes must agree BYTE FOR BYTE: they do the same
rounded fp32 operations in the same order (lstm_q8.hip is compiled without contraction).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from bonito_amd import _lib, decode, synthetic
from bonito_amd.engine import HipEncoder
from oracle import crf_ref, lstm_q8_ref, nn_ref

import lstm_digests as ld
import q8_ref

pytestmark = pytest.mark.gpu


GUARD = 4096
MODES = ("dbg", "last", "inner")          # <LAST, DBG> (sums given), <LAST> (no sums), <> (no h16_out): see the module docstring


def _guarded(nbytes, fill):
    """nbytes of `fill` between two guards of 0xA5 -> (whole buffer, the payload as a uint8 view)."""
    buf = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    buf[GUARD:GUARD + nbytes] = fill
    return buf, buf[GUARD:GUARD + nbytes]


def _guards_intact(buf):
    return bool((buf[:GUARD] == 0xA5).all()) and bool((buf[-GUARD:] == 0xA5).all())


def run_layer(x, w_ih, w_hh, bias, bound, reverse, variant=0, mode="dbg", max_rings=0):
    """One call of the hook. h16 is pre-filled with 0xFFFF (a NaN), the fragments with the sentinel 0x80, both between guards.
    -> (h16 fp16 [T][N][H] or None, fragments flat int8, sums int32 [T][N][4H][2] or None)"""
    x = torch.as_tensor(x)
    T, N, H = x.shape
    lib = _lib.lib()
    xd = x.cuda()
    h16_buf, h16 = _guarded(T * N * H * 2, 0xFF)
    hq_buf, hq = _guarded(T * (N // 16) * q8_ref.nk8(H) * 1024, 0x80)
    sums = torch.zeros(T, N, 4 * H, 2, dtype=torch.int32, device="cuda") if mode == "dbg" else None
    w1, w2, b = (np.ascontiguousarray(a, np.float32) for a in (w_ih, w_hh, bias))
    args = (_lib.ptr(xd), float(bound), w1.ctypes.data_as(C.c_void_p), w2.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p),
            T, N, H, int(reverse), variant, _lib.ptr(h16) if mode != "inner" else None, _lib.ptr(hq),
            _lib.ptr(sums) if sums is not None else None)
    if max_rings:          # the second hook: the same call with the rings of a launch capped
        _lib.check(lib.bh_lstm_q8_layer_split(*args, int(max_rings), _lib.stream_ptr()), "bh_lstm_q8_layer_split")
    else:
        _lib.check(lib.bh_lstm_q8_layer(*args, _lib.stream_ptr()), "bh_lstm_q8_layer")
    assert _guards_intact(h16_buf) and _guards_intact(hq_buf), "a guard of h16 / hq_frag was written"
    if mode == "inner":
        assert bool((h16 == 0xFF).all()), "the instance without fp16 rows wrote some"
    return (h16.cpu().numpy().view(np.float16).reshape(T, N, H) if mode != "inner" else None, hq.cpu().numpy().view(np.int8),
            sums.cpu().numpy() if sums is not None else None)


def check_dbg_run(case, bound, reverse, got):
    """The checker of tests/q8_ref.py on a run with sums: fragments (every real unit written, padding still 0x80), exact sums, hq =
    rint(127 h16); -> the worst cell error."""
    x, w_ih, w_hh, bias = case[:4]
    h16, frag, sums = got
    T, N, H = np.asarray(x).shape
    units = q8_ref.check_fragments(frag, T, N, H)
    return q8_ref.check_layer(x, w_ih, w_hh, bias, bound, reverse, h16, units, sums)


def check_three_modes(case, bound, reverse, variant=0, max_rings=0):
    """The hook's three instances on the same inputs: the DBG run passes the checker; h16 of the <LAST> run and the real units of
    the fragments of both product runs are the DBG run's bytes. -> (worst cell error, the DBG run)"""
    x = np.asarray(case[0])
    T, N, H = x.shape
    dbg = run_layer(*case[:4], bound, reverse, variant, "dbg", max_rings)
    worst = check_dbg_run(case, bound, reverse, dbg)
    last = run_layer(*case[:4], bound, reverse, variant, "last", max_rings)
    inner = run_layer(*case[:4], bound, reverse, variant, "inner", max_rings)
    assert np.array_equal(last[0].view(np.uint16), dbg[0].view(np.uint16)), "h16 of <LAST> differs from <LAST, DBG>"
    for name, run in (("last", last), ("inner", inner)):
        units = q8_ref.check_fragments(run[1], T, N, H)
        assert np.array_equal(units, q8_ref.unscramble(dbg[1], T, N, H)[0]), "hq_frag of mode %s differs from the DBG run" % name
    return worst, dbg


@pytest.mark.parametrize("H,variant,N,reverse,bound", [(384, 0, 32, 0, 1.0), (384, 0, 48, 1, 4.0), (384, 1, 32, 1, 1.0), (384, 2, 32, 0, 1.0), (96, 0, 32, 0, 1.0),
                                                       (128, 0, 16, 1, 3.5), (64, 0, 48, 0, 1.0), (192, 0, 32, 1, 1.0), (256, 0, 16, 0, 1.0),
                                                       (288, 0, 16, 1, 1.0), (512, 0, 16, 0, 1.0)])
def test_q8_layer_integer_sums_exact_and_cell_close(H, variant, N, reverse, bound):
    T = 37
    rng = np.random.default_rng(H + variant)
    w_ih = (rng.standard_normal((4 * H, H)) * rng.uniform(0.02, 0.12, (4 * H, 1))).astype(np.float32)
    w_hh = (rng.standard_normal((4 * H, H)) * rng.uniform(0.02, 0.12, (4 * H, 1))).astype(np.float32)
    bias = (rng.standard_normal(4 * H) * 0.3).astype(np.float32)
    x = np.clip(rng.standard_normal((T, N, H)) * 0.6 * bound, -1.2 * bound, 1.2 * bound).astype(np.float16)
    case = (x, w_ih, w_hh, bias)
    worst = check_dbg_run(case, bound, reverse, run_layer(*case, bound, reverse, variant))      # sums and hq exact (q8_ref.check_layer)
    assert worst < 2e-3, worst        # fp16 rounding of h (4.9e-4) + fast exp / rcp, accumulated through c over 37 steps


BOUNDS = (1.0, 3.5, 4.0)


@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("H,variant", sorted(q8_ref.INSTANCES))
def test_q8_every_instance_product_path_equals_pinned_path(H, variant, reverse):
    """Every row of BH_LSTM_Q8_INSTANCES (and the second widths 192 and 336) in its three LAST / DBG instances at N = 32, T = 11."""
    bound = BOUNDS[(H // 16 + variant + reverse) % 3]
    case = q8_ref.typical_case(H, 11, 32, bound, seed=3 + variant)
    worst, _ = check_three_modes(case, bound, reverse, variant)
    print("H %d variant %d reverse %d bound %.1f: worst cell error %.3g" % (H, variant, reverse, bound, worst))
    assert worst < 2e-3, worst


@pytest.mark.parametrize("reverse", [0, 1])
@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6, 9])
@pytest.mark.parametrize("H", [384, 336, 64])
def test_q8_short_sequences(H, T, reverse):
    """T = 1..6 and 9: the prologue's second x tile (T = 1), the four-slot exchange ring with and without a re-arm (it first happens at
    T = 5), the triple x buffer wrapping once (T = 4..6) and twice (T = 9)."""
    case = q8_ref.typical_case(H, T, 16, 1.0, seed=10 + T)
    worst, _ = check_three_modes(case, 1.0, reverse)
    print("H %d T %d reverse %d: worst cell error %.3g" % (H, T, reverse, worst))
    assert worst < 2e-3, worst


def _same_bytes(a, b):
    return all((u is None and v is None) or np.array_equal(np.asarray(u).view(np.uint8), np.asarray(v).view(np.uint8)) for u, v in zip(a, b))


@pytest.mark.parametrize("H", q8_ref.SERVED)
def test_q8_forced_launch_split(H):
    """Three rings in launches of 1 + 1 + 1, of 2 + 1 (a ragged last launch) and in one launch: identical h16, hq_frag and sums, and
    the checker passes; the two product instances split ring by ring give the same bytes again."""
    reverse = (H // 16) % 2
    bound = BOUNDS[(H // 32) % 3]
    case = q8_ref.typical_case(H, 11, 48, bound, seed=21)
    whole = run_layer(*case, bound, reverse, 0, "dbg", 0)
    worst = check_dbg_run(case, bound, reverse, whole)
    assert worst < 2e-3, worst
    for per in (1, 2):
        assert _same_bytes(run_layer(*case, bound, reverse, 0, "dbg", per), whole), per
    last = run_layer(*case, bound, reverse, 0, "last", 1)
    inner = run_layer(*case, bound, reverse, 0, "inner", 2)
    assert _same_bytes(last[:2], whole[:2]) and np.array_equal(inner[1], whole[1])


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lstm_kernels_parent.json")) as _fh:
    PARENT = json.load(_fh)


def test_q8_kernels_have_the_bytes_of_the_commit_before_the_shared_header():
    """tests/golden/lstm_kernels_parent.json (tools/lstm_kernel_digests.py, cases of tests/lstm_digests.py): every instance in its three
    LAST / DBG forms at T = 5, both directions, and H = 384 at T = 1, 2, 3, 11, 14 - h16, the int8 fragments and the int32 sums."""
    assert PARENT["seed"] == ld.SEED
    want = PARENT["q8"]
    got = {ld.q8_key(*c): ld.q8_digest(*c) for c in ld.q8_cases()}
    assert sorted(got) == sorted(want)
    assert [k for k in got if got[k] != want[k]] == []


@pytest.mark.parametrize("name", [n for n in ld.ENGINE_CASES if n.startswith("q8")])
def test_q8_options_have_the_bytes_of_the_commit_before_the_shared_header(name):
    """What only an encoder passes on to the 8-bit kernel: the "lstm_tune" bit-5 spread over the XCDs and the write-through policy."""
    assert ld.engine_digest(name) == PARENT["engine"][name]


def _rings_per_launch(H, variant=0):
    out = (C.c_int32 * 17)()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _lib.lib().bh_lstm_launch_plan(_lib.LSTM_FAMILIES["q8"], H, variant, 1, cus, out, 17)
    assert out[0] == 1 and out[6] >= 1
    return int(out[6])


def test_q8_launch_boundary_of_the_device():
    """One ring more than a launch holds at H = 384 (528 chunks on an MI355X): the device's own split. Every ring passes the checker,
    and the ring of the second launch gives the bytes of the same 16 chunks run alone."""
    H, T = 384, 6
    per = _rings_per_launch(H)
    N = 16 * (per + 1)
    case = q8_ref.typical_case(H, T, N, 1.0, seed=33)
    got = run_layer(*case, 1.0, 0, 0, "dbg")
    worst = check_dbg_run(case, 1.0, 0, got)
    assert worst < 2e-3, worst
    alone = run_layer(np.ascontiguousarray(case[0][:, -16:]), *case[1:], 1.0, 0, 0, "dbg")
    tile = q8_ref.nk8(H) * 1024
    assert np.array_equal(got[0][:, -16:].view(np.uint16), alone[0].view(np.uint16))
    assert np.array_equal(got[1].reshape(T, N // 16, tile)[:, -1], alone[1].reshape(T, 1, tile)[:, 0])
    assert np.array_equal(got[2][:, -16:], alone[2])
    prod = run_layer(*case, 1.0, 0, 0, "last")
    assert _same_bytes(prod[:2], got[:2])


# measured on MI355X with this test (H = 96 / 384, three bounds, T = 9): the worst |h16 - fp64 cell| is SAT_MEASURED, 1.4e-7 UNDER the
# rounding of h to fp16 alone (half an ulp below 1, 2^-12 = 2.441e-4): what the fast exp / rcp and the fp32 carry of c add does not
# show above that rounding, so their measured share SAT_FAST is zero and the tolerance is the issue's 4.9e-4 + 2 x 0
SAT_MEASURED = 2.440007e-4
SAT_FAST = max(SAT_MEASURED - 2.0 ** -12, 0.0)
SAT_TOL = 4.9e-4 + 2 * SAT_FAST


@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("H", [96, 384])
def test_q8_saturation(H, bound):
    """Gates beyond the clamps of lstm_cell in both signs (biases of +-30 in eight patterns by unit), all-zero weight rows, inputs at
    +-10 bound and +-65504. Sums exact; xq saturates at +-127; hq reaches +127 and -127 and never -128; h16 finite; the cell within
    SAT_TOL = 4.9e-4 (fp16 half-ulp as the project counts it) + 2 x the measured fast-exp / rcp error. Measured on MI355X: worst
    |h16 - fp64 cell| over the six cases 1.824e-4, 2.377e-4, 2.294e-4 (H = 96; bound 1, 3.5, 4) and 2.416e-4, 2.440007e-4, 2.428e-4
    (H = 384): never above the fp16 rounding alone (2^-12 = 2.441e-4), so the fast-math share is 0 and SAT_TOL = 4.9e-4, well inside
    the 2e-3 of the other tests (saturated gates make the cell LESS sensitive to the transcendentals, and T is 9, not 37)."""
    T, N = 9, 16
    reverse = int(bound == 3.5)
    x, w_ih, w_hh, bias, far = q8_ref.saturating_case(H, T, N, bound, seed=H)
    case = (x, w_ih, w_hh, bias)
    xq, want_x = q8_ref.expected_x_sums(x, w_ih, bound)
    assert far.any() and (np.abs(xq[far]) == 127).all() and (xq[far] == 127).any() and (xq[far] == -127).any()
    # an int8 cast without the clip would wrap 10 * bound (1270 -> -10) and lose 65504: the sums tell
    wrapped = np.rint(x.astype(np.float32) * np.float32(127.0 / bound)).astype(np.int64).astype(np.int8)
    assert not np.array_equal(wrapped, xq)
    worst, dbg = check_three_modes(case, bound, reverse)          # exact sums == want_x inside, hq never -128, h16 finite
    assert np.array_equal(dbg[2][..., 0], want_x)
    hq = q8_ref.unscramble(dbg[1], T, N, H)[0]
    assert (hq == 127).any() and (hq == -127).any() and not (hq == -128).any()
    assert np.isfinite(dbg[0].astype(np.float32)).all()
    zero_rows = np.abs(w_hh).max(axis=1) == 0
    assert zero_rows.any() and not dbg[2][:, :, zero_rows, 1].any()
    print("H %d bound %.1f: worst cell error %.7g = 2^-12 %+.3g (tolerance %.4g)" % (H, bound, worst, worst - 2.0 ** -12, SAT_TOL))
    assert worst < SAT_TOL, worst


@pytest.mark.parametrize("H", [384, 144])
def test_q8_engine_scores_do_not_depend_on_the_batch(H):
    """The stack as the product runs it (layers 1..4 write int8 fragments only, q_act ping-pong, padding rows of a batch of 21): the
    scores of 21 chunks are the same bytes in any order and, at H = 384, at either end of a batch one ring past a launch, where the
    engine's own split loop runs."""
    from bonito_amd import nn as bnn
    torch.manual_seed(H)
    model = bnn.from_dict(synthetic.lstm_crf_encoder_config(H, 3)).eval()
    nn_ref.round_params_to_half_(model)
    big = 16 * (_rings_per_launch(H) + 1) if H == 384 else 21
    gen = torch.Generator().manual_seed(H + 1)
    x = torch.randn(21, 1, 900, generator=gen).half().cuda()
    enc = HipEncoder(model, batchsize=big, chunksize=900, quantize=True)
    assert "lstm_layer_q8_kernel" in enc.describe()

    def run(batch):
        out = enc(batch)
        enc.check()
        return out

    want = run(x)
    assert torch.isfinite(want.float()).all()
    perm = torch.randperm(21, generator=gen).cuda()
    assert torch.equal(run(x[perm]), want[perm])
    if H == 384:
        rest = torch.randn(big - 21, 1, 900, generator=gen).half().cuda()
        assert torch.equal(run(torch.cat((x, rest)))[:21], want)
        assert torch.equal(run(torch.cat((rest, x)))[-21:], want)
    enc.close()


def _scores(model, x, quantize):
    enc = HipEncoder(model.encoder, batchsize=x.shape[0], chunksize=x.shape[-1], quantize=quantize)
    out = enc(x.half().cuda())
    enc.check()
    return out, enc


@pytest.mark.parametrize("name,N,L", [("hac", 21, 1800), ("fast", 19, 1800)])
def test_q8_engine_matches_oracle_and_decodes_like_fp32(name, N, L):
    model = synthetic.make_model(name, batchsize=N, chunksize=L)
    nn_ref.round_params_to_half_(model)
    x = torch.randn(N, 1, L, generator=torch.Generator().manual_seed(3)).half()
    got, enc = _scores(model, x, True)
    assert "lstm_layer_q8_kernel" in enc.describe()
    with torch.no_grad():
        ref = nn_ref.forward(model.encoder, x.float(), expand_blanks=False).permute(1, 0, 2)
        q8 = lstm_q8_ref.forward_q8(model.encoder, x.float(), expand_blanks=False).permute(1, 0, 2)
    g = got.cpu().float()
    d_def = (g - q8).abs()              # kernel vs its definition: the integer part is exact, the cell differs by ~1e-3, and a
    d_ref = (g - ref).abs()             # rare flip of a quantisation bucket (1/127) propagates -> a loose bound on max, tight mean
    # measured on MI355X: kernel vs definition max 0.086 / mean 0.010-0.011 (the convolutions ahead of the first recurrent layer
    # run in fp16 on the GPU and in fp32 in the oracle, so ~10 % of its int8 inputs land in the neighbouring bucket)
    assert d_def.mean().item() < 0.03 and d_def.max().item() < 0.3, (d_def.max().item(), d_def.mean().item())      # max: 3.5 x measured
    assert d_ref.max().item() < 0.6 and d_ref.mean().item() < 0.06, (d_ref.max().item(), d_ref.mean().item())
    sl = model.seqdist.state_len
    paths = [crf_ref.viterbi(s.contiguous().numpy().astype(np.float16), sl, blank=2.0)[1] for s in (ref, g)]
    assert (paths[0] == paths[1]).mean() > 0.99
    # the fp16 engine on the same model, for scale
    f16, _ = _scores(model, x, False)
    assert (f16.cpu().float() - ref).abs().max().item() < 3e-2


@pytest.mark.parametrize("H", [64, 96, 128, 144, 192, 256, 288, 320, 336, 384, 448, 480, 512])
def test_quantize_covers_or_falls_back_for_every_width(H):
    """`quantize=True` on any hidden size the ring kernels serve: widths with an 8-bit kernel instance run it, the others keep the
    fp16 kernels (use_hip's contract) - never a failing forward (advisor finding, round 2: the shape predicate accepted widths
    without an instance). Either way the scores stay close to the fp32 oracle."""
    from bonito_amd import nn as bnn
    cfg = synthetic.lstm_crf_encoder_config(H, 3)
    torch.manual_seed(H)
    model = bnn.from_dict(cfg).eval()
    nn_ref.round_params_to_half_(model)
    x = torch.randn(32, 1, 900, generator=torch.Generator().manual_seed(H)).half()
    enc = HipEncoder(model, batchsize=32, chunksize=900, quantize=True)
    got = enc(x.cuda())
    enc.check()
    layout = enc.describe()
    has_q8 = H in q8_ref.SERVED          # 144 and 336: the widths with one real quarter in the last k-step; 320, 448, 480: accepted by the round-2 predicate, no kernel instance
    assert ("lstm_layer_q8_kernel" in layout) == has_q8, layout
    from bonito_amd.crf.basecall import q8_covers
    assert q8_covers(H) == has_q8          # the host-side lane policy (max_lanes) uses the same predicate
    with torch.no_grad():
        ref = nn_ref.forward(model, x.float(), expand_blanks=False).permute(1, 0, 2)
    d = (got.cpu().float() - ref).abs()
    assert d.mean().item() < (0.06 if has_q8 else 8e-3), (H, d.max().item(), d.mean().item())      # fp16 fallback measured: 3.8e-3 at 480


@pytest.mark.parametrize("H", [144, 336])
def test_q8_only_widths_run_quantised_and_nowhere_else(H):
    """144 and 336 have an 8-bit instance and no fp16 one: a quantised model runs, the A/B switch "lstm_q8" = 0 cannot move it to
    kernels that do not exist (same bytes), and without `quantize` bh_encoder_create refuses the model with a message."""
    from bonito_amd import nn as bnn
    torch.manual_seed(H)
    model = bnn.from_dict(synthetic.lstm_crf_encoder_config(H, 3)).eval()
    x = torch.randn(16, 1, 600, generator=torch.Generator().manual_seed(H)).half().cuda()
    enc = HipEncoder(model, batchsize=16, chunksize=600, quantize=True)
    a = enc(x)
    enc.set_option("lstm_q8", 0)
    assert "lstm_layer_q8_kernel" in enc.describe()
    b = enc(x)
    enc.check()
    assert torch.equal(a, b) and torch.isfinite(a.float()).all()
    with pytest.raises(_lib.HipEngineError, match="8-bit kernel serves"):
        HipEncoder(model, batchsize=16, chunksize=600)


def test_q8_option_off_runs_the_fp16_kernels():
    model = synthetic.make_model("hac", batchsize=16, chunksize=1200)
    x = torch.randn(16, 1, 1200, generator=torch.Generator().manual_seed(1)).half().cuda()
    enc = HipEncoder(model.encoder, batchsize=16, chunksize=1200, quantize=True)
    a = enc(x)
    enc.set_option("lstm_q8", 0)
    b = enc(x)
    enc.check()
    plain = HipEncoder(model.encoder, batchsize=16, chunksize=1200)
    assert torch.equal(b, plain(x)) and not torch.equal(a, b)
    assert "q8" not in plain.describe()


def test_q8_full_size_hac_512x10000():
    """BASELINE size with quantize=True: no exchange timeout, finite scores, four chunks of the batch against the Q8-1 oracle
    and the fp32 oracle, decode of the engine's scores bit-exact vs the C oracle; both kernel geometries agree bit for bit."""
    model = synthetic.make_model("hac", batchsize=512, chunksize=10000)
    nn_ref.round_params_to_half_(model)
    x = torch.randn(512, 1, 10000, generator=torch.Generator().manual_seed(25)).half()
    got, enc = _scores(model, x, True)
    assert got.shape == (512, 1667, 1024) and torch.isfinite(got.float()).all()
    rows = [0, 17, 255, 511]
    with torch.no_grad():
        ref = nn_ref.forward(model.encoder, x[rows].float(), expand_blanks=False).permute(1, 0, 2)
        q8 = lstm_q8_ref.forward_q8(model.encoder, x[rows].float(), expand_blanks=False).permute(1, 0, 2)
    g = got[rows].cpu().float()
    d_def, d_ref = (g - q8).abs(), (g - ref).abs()
    assert d_def.mean().item() < 0.02, (d_def.max().item(), d_def.mean().item())
    assert d_ref.mean().item() < 0.08, (d_ref.max().item(), d_ref.mean().item())
    sub = got[rows].cpu().numpy()
    seq, qs, mv = decode.beam_search(got)
    oseq, oqs, omv, _ = crf_ref.beam_search(sub, 4)
    assert np.array_equal(mv.numpy()[rows], omv) and np.array_equal(seq.numpy()[rows], oseq)
    p_ref = crf_ref.viterbi(ref.contiguous().numpy().astype(np.float16), 4, blank=2.0)[1]
    p_q8 = crf_ref.viterbi(sub, 4, blank=2.0)[1]
    assert (p_ref == p_q8).mean() > 0.98
    enc.close()
    try:
        for variant, tag in ((1, "lstm_layer_q8_kernel<6,1>"), (2, "lstm_layer_q8_kernel<6,3>")):
            decode.set_option("lstm_q8_variant", variant)       # 1: 4 units per wave, 3 workgroups per CU; 2: occupancy 2
            alt, enc2 = _scores(model, x, True)
            assert tag in enc2.describe()
            assert torch.equal(alt, got), variant
            enc2.close()
    finally:
        decode.set_option("lstm_q8_variant", 0)

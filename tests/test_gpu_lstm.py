"""Every fp16 recurrent kernel family of csrc/lstm.hip (wave, fused, stream, wgx, wgx2, cta, wide) at operator level (-m gpu):
bh_lstm_layer_family against the teacher-forced fp64 reference of tests/lstm_ref.py, every published element within its a-priori
bound (derived there, pinned by tests/test_lstm_ref_cpu.py; nothing is tuned here). Every run also checks guard halves in front of
and behind h_out, the timeout flag (an error return of the entry) and that a second run gives the same bytes; the exchange policies
(flags bit 0) must agree bit for bit. The references run on the device in fp64."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import lstm_digests as ld
import lstm_ref as lr
from bonito_amd import _lib

pytestmark = pytest.mark.gpu

FAM = _lib.LSTM_FAMILIES
GEMM_FIRST = ("wave", "stream", "wide")                 # G = fp16(x W_ih^T + b) is part of the operation
HAS_POLICY = ld.HAS_POLICY
GUARD, FRONT, BACK = 0x7E5A, 64, 4096                   # an fp16 NaN payload no result can equal (|h| <= 1; the kernels' own sentinel is 0xFFFF)
WIDTHS, MAIN = ld.WIDTHS, ld.MAIN       # (family -> widths with an instance, the width the longer tests use): tests/lstm_digests.py
T_SET = (1, 2, 3, 5, 9, 10, 13, 17)     # the paired kernel's unrolled loop runs for 4 <= step, step + 4 <= T - 2: none, one pass, every tail
WORST = {}                              # (family, class) -> largest err / bound seen


def ring_of(family):
    return 32 if family == "wide" else 16


def launch(family, case, reverse, flags=0):
    """-> int16 bits [T][N][H] of h_out; guards checked."""
    x, w_ih, w_hh, bias = case
    T, N, H = x.shape
    xd = x.cuda()
    buf = torch.full((FRONT + T * N * H + BACK,), GUARD, dtype=torch.int16, device="cuda")
    out = buf[FRONT:FRONT + T * N * H]
    w1, w2 = (np.ascontiguousarray(w.numpy(), np.float32) for w in (w_ih, w_hh))
    b = None if bias is None else np.ascontiguousarray(bias.numpy(), np.float32)
    rc = _lib.lib().bh_lstm_layer_family(_lib.ptr(xd), w1.ctypes.data_as(C.c_void_p), w2.ctypes.data_as(C.c_void_p),
                                         None if b is None else b.ctypes.data_as(C.c_void_p), T, N, H, int(reverse), FAM[family], flags,
                                         C.c_void_p(out.data_ptr()), _lib.stream_ptr())
    _lib.check(rc, "bh_lstm_layer_family(%s, H=%d, T=%d, N=%d, flags=%d)" % (family, H, T, N, flags))      # (a timeout is an error return)
    torch.cuda.synchronize()
    assert (buf[:FRONT] == GUARD).all() and (buf[FRONT + T * N * H:] == GUARD).all(), "%s H=%d: guard halves of h_out overwritten" % (family, H)
    return out.view(T, N, H).clone()


def judge(family, cls, case, bits, reverse):
    x, w_ih, w_hh, bias = case
    got = bits.view(torch.float16)
    want, bound = lr.teacher_forced(x.cuda(), w_ih.cuda(), w_hh.cuda(), None if bias is None else bias.cuda(), got, reverse,
                                    gemm=family in GEMM_FIRST)
    ratio, (t, n, u) = lr.worst(got, want, bound)
    T = x.shape[0]
    WORST[(family, cls)] = max(WORST.get((family, cls), 0.0), ratio)
    print("%s H=%d T=%d N=%d %s %s: worst err / bound %.3f" % (family, x.shape[2], T, x.shape[1], cls, "rev" if reverse else "fwd", ratio))
    assert ratio <= 1.0, ("%s H=%d T=%d %s %s: err / bound = %.3g at time %d (step %d), ring %d (column %d), unit %d: got %r want %r bound %.3g"
                          % (family, x.shape[2], T, cls, "reverse" if reverse else "forward", ratio, t, T - 1 - t if reverse else t,
                             n // ring_of(family), n, u, float(got[t, n, u]), float(want[t, n, u]), float(bound[t, n, u])))
    if cls == "zeros":
        assert (bits == 0).all(), "%s H=%d: x = 0 without bias must give +0 everywhere" % (family, x.shape[2])


def run(family, cls, T, N, H, reverse, seed=0, replicate=False, modes=(0,)):
    """One case: every mode of `modes` (flags) twice, all bytes equal, judged against the reference. -> the bits."""
    case = lr.make_case(cls, T, N, H, seed=seed, replicate=replicate)
    first = launch(family, case, reverse, modes[0])
    for flags in modes:
        again = launch(family, case, reverse, flags)
        assert torch.equal(first, again), "%s H=%d T=%d %s: flags %d differ from a first run with flags %d" % (family, H, T, cls, flags, modes[0])
    judge(family, cls, case, first, reverse)
    return first


def modes_of(family):
    if family == "wide":
        return (0, 1, 2, 3)              # ring-buffer and output-tensor hand-off, each with both store policies
    return (0, 1) if family in HAS_POLICY else (0,)


INSTANCES = [(f, H) for f in WIDTHS for H in WIDTHS[f]]


@pytest.mark.parametrize("family,H", INSTANCES, ids=["%s-%d" % i for i in INSTANCES])
def test_every_instance(family, H):
    """One ring and three rings (an odd count: a lone ring in wgx2's last workgroups, a part-filled slot of four in wave and fused),
    both directions, typical / saturating / zeros data, every hand-off and store policy."""
    r = ring_of(family)
    for k, cls in enumerate(("typical", "saturating", "zeros")):
        for rings in (1, 3):
            run(family, cls, 13, rings * r, H, reverse=(k + rings) % 2 == 1, seed=H, modes=modes_of(family))
    run(family, "typical", 13, 3 * r, H, reverse=True, seed=H + 1)
    run(family, "saturating", 13, r, H, reverse=True, seed=H + 1)


@pytest.mark.parametrize("reverse", [False, True], ids=["fwd", "rev"])
@pytest.mark.parametrize("family,H", [(f, MAIN[f]) for f in MAIN] + [("wgx2", 256), ("wgx2", 96), ("wgx", 256)],
                         ids=lambda v: str(v))
def test_every_length(family, H, reverse):
    for T in T_SET:
        run(family, "typical" if T % 2 else "long_memory", T, 3 * ring_of(family), H, reverse, seed=T, modes=modes_of(family)[:2])


@pytest.mark.parametrize("cls", [c for c in lr.CLASSES if c != "zeros"])
@pytest.mark.parametrize("family", list(MAIN))
def test_four_hundred_steps(family, cls):
    """T = 400 at the family's main width: saturating lets c climb past the clamp inside tanh(c), long_memory carries c throughout."""
    H = MAIN[family]
    reverse = lr.CLASSES.index(cls) % 2 == 1
    run(family, cls, 400, 3 * ring_of(family), H, reverse, seed=400)
    if cls == "typical":                 # sanity at the old tolerance of test_lstm_layer: the free-running recurrence
        case = lr.make_case(cls, 400, 3 * ring_of(family), H, seed=400)
        got = launch(family, case, reverse).view(torch.float16)
        free = lr.free_running(case[0].cuda(), case[1].cuda(), case[2].cuda(), case[3].cuda(), reverse)
        assert (got.double() - free).abs().max().item() < 6e-3


@pytest.mark.parametrize("family", list(MAIN))
def test_columns_are_independent(family):
    """The same chunk in every batch column: every column must carry the same bytes (ring and slot indexing that the comparison with
    the reference could excuse element by element)."""
    for cls, reverse in (("typical", False), ("saturating", True)):
        bits = run(family, cls, 17, 3 * ring_of(family), MAIN[family], reverse, seed=5, replicate=True)
        assert (bits == bits[:, :1]).all(), "%s: columns of one replicated chunk differ" % family


@pytest.mark.parametrize("H", [64, 96, 128, 192, 256, 288, 384])
def test_fused_families_agree_bit_for_bit(H):
    """fused, wgx, wgx2 (and cta where it has an instance) compute the same pre-activations in the same order and share lstm_cell()."""
    fams = ["fused", "wgx", "wgx2"] + (["cta"] if H in WIDTHS["cta"] else [])
    for cls, T, reverse in (("typical", 17, False), ("saturating", 17, True), ("overflow", 10, False)):
        case = lr.make_case(cls, T, 48, H, seed=H)
        ref = launch(fams[0], case, reverse)
        judge(fams[0], cls, case, ref, reverse)
        for f in fams[1:]:
            assert torch.equal(launch(f, case, reverse), ref), "%s differs from fused at H=%d on %s data" % (f, H, cls)


@pytest.mark.parametrize("H", list(range(576, 1025, 64)))
def test_every_wide_width_runs_or_is_refused_at_create(H):
    """Every multiple of 64 in (512, 1024]: the engine either refuses the model at create or runs it - never a failing forward
    (576, 704, 832 and 960 used to pass create and fail the first forward with "unsupported H": the streaming kernel had no
    instance). What it runs meets the bound at operator level (test_every_instance[stream-H]); here, the scores against the
    fp32 oracle at the tolerance the other widths have."""
    from bonito_amd import nn as bnn, synthetic
    from bonito_amd.engine import HipEncoder
    from oracle import nn_ref
    cfg = synthetic.lstm_crf_encoder_config(H, 3, n_lstm=2)
    torch.manual_seed(H)
    model = bnn.from_dict(cfg).eval()
    nn_ref.round_params_to_half_(model)
    x = torch.randn(16, 1, 600, generator=torch.Generator().manual_seed(H)).half()
    try:
        enc = HipEncoder(model, batchsize=16, chunksize=600)
    except _lib.HipEngineError:
        return
    got = enc(x.cuda())
    enc.check()
    assert ("lstm_layer_wide_kernel" in enc.describe()) == (H % 128 == 0), enc.describe()
    with torch.no_grad():
        ref = nn_ref.forward(model, x.float(), expand_blanks=False).permute(1, 0, 2)
    d = (got.cpu().float() - ref).abs()
    assert torch.isfinite(got.float()).all() and d.max().item() < 2.4e-2 and d.mean().item() < 8e-3, (H, d.max().item(), d.mean().item())


with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lstm_kernels_parent.json")) as _fh:
    PARENT = json.load(_fh)


@pytest.mark.parametrize("family", list(WIDTHS))
def test_every_family_has_the_bytes_of_the_commit_before_the_shared_header(family):
    """tests/golden/lstm_kernels_parent.json: digests written by tools/lstm_kernel_digests.py against a build of the commit before the
    recurrent kernels moved their shared parts into csrc/lstm_ring.h. Cases: tests/lstm_digests.py."""
    assert PARENT["seed"] == ld.SEED
    want = PARENT["fp16"][family]
    got = {ld.fp16_key(*c): ld.fp16_digest(family, *c) for c in ld.fp16_cases(family)}
    assert sorted(got) == sorted(want)
    assert [k for k in got if got[k] != want[k]] == []


@pytest.mark.parametrize("name", [n for n in ld.ENGINE_CASES if not n.startswith("q8")])
def test_tune_bits_have_the_bytes_of_the_commit_before_the_shared_header(name):
    """The "lstm_tune" bits only an encoder passes on: the bit-5 spread over the XCDs (wgx, wgx2, wide) and wgx2's generic section code.
    The digest is of a whole encoder's scores (tests/lstm_digests.py, engine_digest): a change on purpose to the convolutions, the linear
    layer, the CRF head or the model builder moves it too, and the golden is then rewritten from the commit before that change."""
    assert ld.engine_digest(name) == PARENT["engine"][name]


def test_zz_worst_ratio_per_family_and_class():
    """Reports the largest err / bound per family and data class seen by the tests above (DESIGN.md section 6 quotes a full run)."""
    for (family, cls), r in sorted(WORST.items()):
        print("lstm worst err/bound  %-7s %-12s %.3f" % (family, cls, r))
        assert r <= 1.0

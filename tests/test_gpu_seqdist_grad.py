"""Gradients of the CTC-CRF log-sums on the device (-m gpu): bh_crf_seq_logz_grad / bh_crf_logz_dense_grad, decode.seq_logz_grad /
logz_grad, CTC_CRF.posteriors and the autograd of CTC_CRF.ctc_loss / SeqdistModel.loss against the fp64 alpha-beta restatement
(tests/seqdist_grad_ref.py).

TOLERANCE. Nothing is fixed in advance, as in tests/test_gpu_seqdist.py. On the SAME inputs (and the same weights) the restatement is run
in fp32, in the reference's order, and compared with its fp64 run: g32 = the largest absolute distance over the elements of the case. A
kernel is allowed, per element,
    4 x g32                                   it sums in another order and uses the hardware exp / log
  + 2^-30 x share x |weight|                  chain gradient only: the fixed-point combine; share = the largest number of chain edges of
                                              the chunk that gather one element
  + 2^-11 |v| + 2^-24  (fp16 output)  or  2^-23 |v|  (fp32 output)        the rounding of the written value v.
Every test prints g32 and the kernel's distance; the measured figures are recorded in DESIGN.md section 6."""
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
import seqdist_cases as sc_cases
import seqdist_ref as sr
import seqdist_grad_ref as gr
from bonito_amd import decode
from bonito_amd.crf.model import CTC_CRF, SeqdistModel

pytestmark = pytest.mark.gpu

ALPHABET = ["N", "A", "C", "G", "T"]
FIXTURE_CASES = ["sl1_koi", "sl2_koi", "sl3_koi", "sl4_koi", "sl5_koi", "sl1_5s", "sl2_5s", "sl3_5s"]


def _rounding(v, dtype):
    v = np.abs(v)
    return 2.0 ** -11 * v + 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -23 * v


def _ntc(x, five):
    """device / host tensor in its own layout -> numpy indexed [n, t, c]"""
    a = x.detach().cpu().numpy()
    return a.transpose(1, 0, 2) if five else a


@functools.lru_cache(maxsize=None)
def _fixture(name):
    """One fixture case with its references, computed once: fp64 truth and the fp32 reference-order run of both gradients."""
    z = np.load(os.path.join(GOLDEN, "crf_ctc_loss.npz"))
    sl, five = int(name[2]), name.endswith("_5s")
    raw = z[name + "/scores"]
    c = {"sl": sl, "five": five, "raw": raw, "ntc": raw.transpose(1, 0, 2) if five else raw, "blank": None if five else 2.0,
         "targets": z[name + "/targets"], "lengths": z[name + "/lengths"], "clip": float(z["loss_clip"])}
    args = (c["ntc"], c["targets"], c["lengths"], sl, five, c["blank"])
    c["chain64"], c["chain32"] = gr.chain_grad(*args), gr.chain_grad(*args, dtype=np.float32)
    c["lz64"], c["dense64"] = gr.dense_grad(c["ntc"], sl, five, c["blank"])
    _, dense32 = gr.dense_grad(c["ntc"], sl, five, c["blank"], dtype=np.float32)
    c["g32_chain"] = float(np.abs(c["chain32"]["grad"].astype(np.float64) - c["chain64"]["grad"]).max())
    c["g32_dense"] = float(np.abs(dense32.astype(np.float64) - c["dense64"]).max())
    for v in (c["chain64"]["grad"], c["chain32"]["grad"], c["chain64"]["logz"], c["dense64"], c["lz64"]):
        v.setflags(write=False)                                                          # shared among the tests: left unchanged
    return c


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_fixture_chain_and_dense_gradient(name):
    """Measured on MI355X: see DESIGN.md section 6 (g32 and the kernel distance per case)."""
    c = _fixture(name)
    sl, five, blank = c["sl"], c["five"], c["blank"]
    x = torch.from_numpy(c["raw"]).cuda()
    tg, ln = torch.from_numpy(c["targets"]), torch.from_numpy(c["lengths"])
    fin = np.isfinite(c["chain64"]["logz"])
    assert fin.any() and (~fin).any()
    plain = decode.seq_logz(x, tg, ln, sl, blank)
    for xin, targets in ((x, tg), (x, tg.to(torch.int32)), (x.float(), tg)):          # int8 / int32 rows, fp16 / fp32 scores and gradients
        logz, g = decode.seq_logz_grad(xin, targets, ln, sl, blank)
        assert g.dtype == xin.dtype and g.shape == xin.shape
        assert torch.equal(logz, plain)                                               # bit for bit the forward scan, -inf included
        got = _ntc(g, five).astype(np.float64)
        want = c["chain64"]["grad"]
        bound = 4 * c["g32_chain"] + 2.0 ** -30 * c["chain64"]["share"][:, None, None] + _rounding(want, xin.dtype)
        dk = float(np.abs(got - want).max())
        print("%s chain (%s): g32 %.3e kernel %.3e" % (name, str(xin.dtype)[6:], c["g32_chain"], dk))
        assert not got[~fin].any()                                                    # the target does not fit: exactly zero
        assert (np.abs(got - want) <= bound).all(), (dk, c["g32_chain"])
    for xin in (x, x.float()):
        lz, g = decode.logz_grad(xin, sl, blank)
        assert g.dtype == xin.dtype and g.shape == xin.shape
        if five:                                                                      # (contiguous koi scores take bh_crf_logz there)
            assert torch.equal(lz.double(), decode.logz_any(x, sl, blank))
        got = _ntc(g, five).astype(np.float64)
        dk = float(np.abs(got - c["dense64"]).max())
        print("%s dense (%s): g32 %.3e kernel %.3e" % (name, str(xin.dtype)[6:], c["g32_dense"], dk))
        assert (np.abs(got - c["dense64"]) <= 4 * c["g32_dense"] + _rounding(c["dense64"], xin.dtype)).all(), (dk, c["g32_dense"])
        assert np.abs(lz.cpu().numpy() - c["lz64"]).max() <= 1e-4 * np.abs(c["lz64"]).max()


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_fixture_ctc_loss_backward(name, dtype):
    """ctc_loss(...).backward(): upstream_n * clip_mask_n / len_n * (post_dense - post_chain); the value bit-equal to the no-grad path."""
    c = _fixture(name)
    sl, five, blank = c["sl"], c["five"], c["blank"]
    sd = CTC_CRF(sl, ALPHABET)
    base = torch.from_numpy(c["raw"]).cuda().to(dtype)
    tg, ln = torch.from_numpy(c["targets"]), torch.from_numpy(c["lengths"])
    lens = c["lengths"].astype(np.float64)
    N = len(lens)
    fin = np.isfinite(c["chain64"]["logz"])
    share = c["chain64"]["share"].astype(np.float64)
    up = np.array([0.75, -1.25, 2.0, 1.0][:N])
    for norm in (True, False):
        D = (c["dense64"] if norm else 0.0) - c["chain64"]["grad"]
        mag = (c["dense64"] if norm else 0.0) + c["chain64"]["grad"]
        err = 4 * c["g32_chain"] + (4 * c["g32_dense"] if norm else 0.0) + 2.0 ** -30 * share[:, None, None] + 2.0 ** -22 * mag
        loss64 = -(c["chain64"]["logz"] - (c["lz64"] if norm else 0.0)) / lens
        for reduction, clip in (("none", None), ("mean", None), ("none", c["clip"]), ("mean", c["clip"]), ("none", 3.0)):
            x = base.clone().requires_grad_(True)
            kw = dict(loss_clip=clip, reduction=reduction, normalise_scores=norm, blank_score=blank)
            loss = sd.ctc_loss(x, tg, ln, **kw)
            with torch.no_grad():
                assert torch.equal(loss.detach(), sd.ctc_loss(base, tg, ln, **kw))      # bit-equal to the no-grad path
            if reduction == "none":
                assert np.isposinf(loss.detach().cpu().numpy()[~fin]).all() or clip
                loss.backward(torch.from_numpy(up).to(loss))
                w = up.copy()
            else:
                loss.backward()
                w = np.full(N, 1.0 / N)
            keep = fin.copy()
            if clip:
                assert np.abs(loss64[fin] - clip).min() > 1e-3                           # no chunk sits on the edge of the clamp
                keep &= (loss64 >= 0) & (loss64 <= clip)
            w = np.where(keep, w / lens, 0.0)
            want = D * w[:, None, None]
            assert x.grad.dtype == dtype and x.grad.shape == x.shape
            got = _ntc(x.grad, five).astype(np.float64)
            assert not got[~keep].any()                                                  # clipped and unreachable chunks: exactly zero
            bound = err * np.abs(w)[:, None, None] + _rounding(want, dtype)
            dk = float(np.abs(got - want).max())
            print("%s %s norm=%d %s clip=%s: g32 chain %.3e dense %.3e, backward vs fp64 %.3e"
                  % (name, str(dtype)[6:], norm, reduction, clip, c["g32_chain"], c["g32_dense"], dk))
            assert (np.abs(got - want) <= bound).all(), dk
        assert keep.any() or not norm                                                    # (clip 3.0 keeps a chunk of every normalised case)


def _geometry_case(npos):
    """state_len 1, [T, N, 20]: a homopolymer row and a random row of npos labels, T = npos + 3."""
    T = npos + 3
    g = torch.Generator(device="cuda").manual_seed(700 + npos)
    x = torch.empty((T, 2, 20), dtype=torch.float16, device="cuda").normal_(0.0, 1.0, generator=g)
    rng = np.random.default_rng(npos)
    targets = rng.integers(1, 5, size=(2, npos)).astype(np.int8)
    targets[0] = 3
    return x, targets, np.array([npos, npos], np.int32)


@pytest.mark.parametrize("npos", sc_cases.NPOS)
def test_geometry_every_positions_per_thread(npos):
    """C = 20, so repeated elements are everywhere: every single-wave P (1, 2, 4, 8) and every four-wave P (4, 8, 16) is hit, each at
    its first and last size - the sizes of seqdist_cases.NPOS, which the forward scans sweep too (an earlier list of its own left
    out 256, 257 and 2049: the last size of 64 x 4 and the first of 64 x 8 and of 256 x 16). State_len 1, the [T, N, 5S] layout, equal
    lengths and unit weights only: test_instance_sweep... below takes the other layout, k-mers, short rows and the flags there."""
    x, targets, lengths = _geometry_case(npos)
    ntc = _ntc(x, True)
    r64 = gr.chain_grad(ntc, targets, lengths, 1, True)
    r32 = gr.chain_grad(ntc, targets, lengths, 1, True, dtype=np.float32)
    g32 = float(np.abs(r32["grad"].astype(np.float64) - r64["grad"]).max())
    assert np.isfinite(r64["logz"]).all() and r64["share"][0] == npos          # the homopolymer: every stay edge on one element, every move edge on another
    logz, g = decode.seq_logz_grad(x, torch.from_numpy(targets), torch.from_numpy(lengths), 1)
    assert torch.equal(logz, decode.seq_logz(x, torch.from_numpy(targets), torch.from_numpy(lengths), 1))
    got = _ntc(g, True).astype(np.float64)
    bound = 4 * g32 + 2.0 ** -30 * r64["share"][:, None, None] + _rounding(r64["grad"], torch.float16)
    dk = float(np.abs(got - r64["grad"]).max())
    print("npos %d: g32 %.3e kernel %.3e (share %s)" % (npos, g32, dk, r64["share"].tolist()))
    assert (np.abs(got - r64["grad"]) <= bound).all(), (dk, g32)
    if npos in (1025, 4096):                                                            # determinism: bit-identical from call to call
        again = decode.seq_logz_grad(x, torch.from_numpy(targets), torch.from_numpy(lengths), 1)[1]
        assert torch.equal(g, again)
        f32 = torch.zeros(x.shape, dtype=torch.float32, device="cuda")
        a = decode.seq_logz_grad(x, torch.from_numpy(targets), torch.from_numpy(lengths), 1, out=f32)[1].clone()
        b = decode.seq_logz_grad(x, torch.from_numpy(targets), torch.from_numpy(lengths), 1, out=f32)[1]
        assert torch.equal(a, b)


def _strided(N, T, C, time_major, gen_seed, pad=8, offset=24):
    """Seeded scores in a padded, offset buffer: the view handed to the kernels is neither contiguous nor at the start of its buffer."""
    g = torch.Generator(device="cuda").manual_seed(gen_seed)
    a, b = (T, N) if time_major else (N, T)
    buf = torch.empty(offset + a * b * (C + pad), dtype=torch.float16, device="cuda")
    buf.normal_(0.0, 2.0, generator=g).clamp_(-5, 5)
    return buf[offset:].as_strided((a, b, C), (b * (C + pad), C + pad, 1))


def _guarded_out(shape, dtype, fill, pad=6, offset=10):
    """A strided, offset gradient view inside a buffer filled with `fill`: (buffer, view, mask of the buffer elements the view covers)."""
    a, b, C = shape
    buf = torch.full((offset + a * b * (C + pad) + 16,), fill, dtype=dtype, device="cuda")
    view = buf[offset:].as_strided((a, b, C), (b * (C + pad), C + pad, 1))
    mask = torch.zeros(buf.shape, dtype=torch.bool, device="cuda")
    mask[offset:].as_strided((a, b, C), (b * (C + pad), C + pad, 1)).fill_(True)
    return buf, view, mask


@pytest.mark.parametrize("five", [False, True], ids=["koi", "5S"])
@pytest.mark.parametrize("sl", [3, 4, 5])
def test_strided_views_guards_and_accumulate(sl, five):
    """T in {1, 5, 67}, N = 5, lengths from state_len up to a target that does not fit; padded, offset, strided scores; a strided `out`
    with guard elements around it; overwrite zeroes what no edge gathers (the buffer is pre-filled), accumulate adds into it."""
    N, S = 5, 4 ** sl
    C = (5 if five else 4) * S
    blank = None if five else 2.0
    for T in (1, 5, 67):
        x = _strided(N, T, C, five, 90 + sl + T)
        Lmax = sl + T + 1
        rng = np.random.default_rng(sl * 100 + T)
        # one that cannot fit, the shortest, ..., one that fits with a move at every step (a homopolymer)
        lengths = np.array([Lmax, sl, min(sl + 1, Lmax - 1), sl + (T + 1) // 2, Lmax - 1], np.int32)
        targets = rng.integers(1, 5, size=(N, Lmax)).astype(np.int8)
        targets[4] = targets[4, 0]
        targets[np.arange(Lmax)[None, :] >= lengths[:, None]] = 0
        wt = np.array([1.0, -1.0, 0.5, 2.0, -0.25])
        ntc = _ntc(x, five)
        r64 = gr.chain_grad(ntc, targets, lengths, sl, five, blank, weight=wt)
        r32 = gr.chain_grad(ntc, targets, lengths, sl, five, blank, weight=wt, dtype=np.float32)
        g32 = float(np.abs(r32["grad"].astype(np.float64) - r64["grad"]).max())
        _, d64 = gr.dense_grad(ntc, sl, five, blank, weight=wt)
        _, d32 = gr.dense_grad(ntc, sl, five, blank, weight=wt, dtype=np.float32)
        gd32 = float(np.abs(d32.astype(np.float64) - d64).max())
        fin = np.isfinite(r64["logz"])
        assert (~fin).sum() == 1 and not fin[0]
        tg = torch.from_numpy(targets).to(torch.int32 if T == 5 else torch.int8)
        ln, w = torch.from_numpy(lengths), torch.from_numpy(wt)
        plain = decode.seq_logz(x, tg, ln, sl, blank)
        fix = 2.0 ** -30 * (r64["share"] * np.abs(wt))[:, None, None]
        worst = [0.0, 0.0]
        for dtype in (torch.float16, torch.float32):
            for accumulate in (False, True):
                fill = 3.0
                buf, out, mask = _guarded_out(x.shape, dtype, fill)
                logz, g = decode.seq_logz_grad(x, tg, ln, sl, blank, weight=w, out=out, accumulate=accumulate)
                assert g is out and torch.equal(logz, plain)
                assert bool((buf[~mask] == fill).all()), "guard elements around the strided gradient were written"
                want = r64["grad"] + (fill if accumulate else 0.0)
                got = _ntc(out, five).astype(np.float64)
                assert (got[~fin] == (fill if accumulate else 0.0)).all()                # no alignment: nothing added / zeros
                untouched = r64["grad"] == 0
                assert (got[untouched] == (fill if accumulate else 0.0)).all()           # overwrite zeroes what no edge gathers
                worst[0] = max(worst[0], float(np.abs(got - want).max()))
                assert (np.abs(got - want) <= 4 * g32 + fix + _rounding(want, dtype)).all(), (T, dtype, accumulate)
            buf, out, mask = _guarded_out(x.shape, dtype, 3.0)
            lz, g = decode.logz_grad(x, sl, blank, weight=w, out=out)
            assert g is out and bool((buf[~mask] == 3.0).all())
            got = _ntc(out, five).astype(np.float64)
            worst[1] = max(worst[1], float(np.abs(got - d64).max()))
            assert (np.abs(got - d64) <= 4 * gd32 + _rounding(d64, dtype)).all(), (T, dtype)
            assert torch.equal(lz.double(), decode.logz_any(x, sl, blank))               # (strided views take the dense scan there too)
        print("sl %d %s T %d: chain g32 %.3e kernel %.3e; dense g32 %.3e kernel %.3e" % (sl, "5S" if five else "koi", T, g32, worst[0], gd32, worst[1]))


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_posteriors(name):
    """CTC_CRF.posteriors = the fp64 dense restatement within the bound; on the [T, N, 5S] fixtures the restatement is first checked against
    the reference's own expression (autograd of its logZ scan, fp64, CPU)."""
    c = _fixture(name)
    sd = CTC_CRF(c["sl"], ALPHABET)
    if c["five"]:
        ref = gr.torch_dense_posteriors(c["raw"], c["sl"]).transpose(1, 0, 2)
        assert np.abs(ref - c["dense64"]).max() < 1e-9
    x = torch.from_numpy(c["raw"]).cuda()
    post = sd.posteriors(x, blank_score=c["blank"])
    assert post.shape == x.shape and post.dtype == x.dtype
    got = _ntc(post, c["five"]).astype(np.float64)
    dk = float(np.abs(got - c["dense64"]).max())
    print("%s posteriors: g32 %.3e kernel %.3e" % (name, c["g32_dense"], dk))
    assert (np.abs(got - c["dense64"]) <= 4 * c["g32_dense"] + _rounding(c["dense64"], torch.float16)).all()
    if c["five"]:
        C = got.shape[2]                                                                 # a step's posteriors sum to 1
        assert np.abs(got.sum(axis=2) - 1.0).max() <= 4 * c["g32_dense"] * C + 2.0 ** -11 + C * 2.0 ** -24


def test_autograd_through_a_linear_layer():
    """A tiny Linear(16, 5 * 4^2) on the device feeds permuted fp16 scores into SeqdistModel.loss(...).backward(): weight.grad against the
    fp64 chain rule through the restatement; the per-element bound of the score gradient is propagated through the matmul (sum |x|)."""
    sl, N, T = 2, 3, 21
    torch.manual_seed(3)
    lin = torch.nn.Linear(16, 5 * 16).cuda()
    feats = torch.randn(N, T, 16, device="cuda")
    model = SeqdistModel(torch.nn.Sequential(), CTC_CRF(sl, ALPHABET))
    rng = np.random.default_rng(8)
    lengths = np.array([2, 9, 17], np.int32)
    targets = rng.integers(1, 5, size=(N, 17)).astype(np.int8)
    targets[np.arange(17)[None, :] >= lengths[:, None]] = 0
    scores = (lin(feats) * 4.0).half().permute(1, 0, 2)                                 # [T, N, 80], a non-contiguous view
    assert not scores.is_contiguous() and scores.requires_grad
    loss = model.loss(scores, torch.from_numpy(targets), torch.from_numpy(lengths))
    loss.backward()
    ntc = _ntc(scores, True)
    args = (ntc, targets, lengths, sl, True, None)
    c64, c32 = gr.chain_grad(*args), gr.chain_grad(*args, dtype=np.float32)
    _, d64 = gr.dense_grad(ntc, sl, True)
    _, d32 = gr.dense_grad(ntc, sl, True, dtype=np.float32)
    g32c = float(np.abs(c32["grad"].astype(np.float64) - c64["grad"]).max())
    g32d = float(np.abs(d32.astype(np.float64) - d64).max())
    w = 1.0 / (N * lengths.astype(np.float64))
    gs = (d64 - c64["grad"]) * w[:, None, None]                                          # d loss / d scores, [n, t, c]
    per = (4 * g32c + 4 * g32d + 2.0 ** -30 * c64["share"][:, None, None] + 2.0 ** -22 * (d64 + c64["grad"])) * w[:, None, None] \
        + _rounding(gs, torch.float16)
    xs = feats.cpu().numpy().astype(np.float64)
    want = 4.0 * np.einsum("ntc,nti->ci", gs, xs)
    # the cast and the scale pass the fp16 gradient on exactly (x 4 is exact); the fp32 matmul adds its own rounding
    bound = 4.0 * np.einsum("ntc,nti->ci", per, np.abs(xs)) + 4.0 * 2.0 ** -22 * np.einsum("ntc,nti->ci", np.abs(gs), np.abs(xs))
    got = lin.weight.grad.cpu().numpy().astype(np.float64)
    dk = float(np.abs(got - want).max())
    print("linear: g32 chain %.3e dense %.3e; weight.grad vs fp64 chain rule %.3e (bound %.3e .. %.3e)" % (g32c, g32d, dk, bound.min(), bound.max()))
    assert np.isfinite(float(loss)) and (np.abs(got - want) <= bound).all(), dk
    want_loss = (-(c64["logz"] - gr.dense_grad(ntc, sl, True)[0]) / lengths).mean()
    assert abs(float(loss) - want_loss) <= 1e-4 * abs(want_loss)


def _loss64(x16, c):
    ok = np.isfinite(c["chain64"]["logz"])
    ntc = _ntc(x16, c["five"])[ok]
    lz = sr.log_scan(ntc, c["targets"][ok], c["lengths"][ok], c["sl"], c["five"], c["blank"])
    return float(((sr.dense_logz(ntc, c["sl"], c["five"], c["blank"]) - lz) / c["lengths"][ok]).sum())


def test_gradient_steps_lower_the_fp64_loss():
    """Ten plain gradient steps (rate 0.5) on the scores of one fixture case lower the fp64 loss of the chunks that fit at every step. The
    restatement's own fp64 descent at that rate does so too (checked first, on the CPU): the rate is small enough."""
    c = _fixture("sl2_5s")
    ok = np.isfinite(c["chain64"]["logz"])
    rate = 0.5
    # the CPU descent with the restatement's gradient, on fp32 master scores rounded to fp16 for the loss exactly as on the device
    master = torch.from_numpy(c["raw"]).float()
    prev = _loss64(master.half(), c)
    for _ in range(10):
        ntc = _ntc(master.half(), True)
        g = (gr.dense_grad(ntc, c["sl"], True)[1] - gr.chain_grad(ntc, c["targets"], c["lengths"], c["sl"], True)["grad"]) \
            * np.where(ok, 1.0 / c["lengths"], 0.0)[:, None, None]
        master -= rate * torch.from_numpy(g.transpose(1, 0, 2)).float()
        now = _loss64(master.half(), c)
        assert now < prev
        prev = now
    sd = CTC_CRF(c["sl"], ALPHABET)
    tg, ln = torch.from_numpy(c["targets"]), torch.from_numpy(c["lengths"])
    x = torch.from_numpy(c["raw"]).float().cuda().requires_grad_(True)
    trace = [_loss64(x.detach().half(), c)]
    for _ in range(10):
        x.grad = None
        loss = sd.ctc_loss(x, tg, ln, reduction="none")
        loss.backward(torch.ones_like(loss))
        assert not x.grad[:, ~torch.from_numpy(ok)].any()
        with torch.no_grad():
            x -= rate * x.grad
        trace.append(_loss64(x.detach().half(), c))
    print("fp64 loss over ten steps: " + " ".join("%.4f" % v for v in trace))
    assert all(b < a for a, b in zip(trace, trace[1:])), trace


# ---- every instance, layout and row class (cases of tests/seqdist_cases.py; tests/test_seqdist_grad_cpu.py proves what they reach) ------
def _chain_refs(ntc, targets, lengths, sl, five, wt):
    """fp64 truth and g32 of one case through the banded restatement (bit for bit chain_grad, see its CPU test)."""
    args = (ntc, targets, lengths, sl, five, None if five else sc_cases.BLANK)
    r64 = gr.chain_grad_banded(*args, weight=wt)
    r32 = gr.chain_grad_banded(*args, weight=wt, dtype=np.float32)
    return r64, float(np.abs(r32["grad"].astype(np.float64) - r64["grad"]).max())


def _chain_bound(r64, g32, wt, want, dtype):
    return 4 * g32 + 2.0 ** -30 * (r64["share"] * np.abs(wt))[:, None, None] + _rounding(want, dtype)


@pytest.mark.parametrize("five", [False, True], ids=["koi", "5S"])
@pytest.mark.parametrize("npos", sc_cases.NPOS)
def test_instance_sweep_layouts_short_rows_and_flags(npos, five):
    """grad_instance_case: state_len 2 (real k-mer gather offsets; C = 80 / 64, so most elements have no owner at small sizes and the
    homopolymer piles every edge on two of them), both layouts, weights 1, -1, 0.5, 0, 2, and next to the full-length rows one of k
    and one of k + 1 labels, which run in whatever instance Lmax selects. logz bit-equal to the forward scan, the weight-0 row exactly
    zero, in the 5S layout every step's gradient sums to the row's weight. At the first size of each instance: fp32 output, int32
    targets, a NaN-filled `out` that comes back finite with exact zeros where the fp64 gradient is zero, and accumulate into a strided
    `out` with guard elements. At 257 and 2049 positions (the first sizes of 64 x 8 and of 256 x 16, the one instance with a prefetch
    depth of 2): equal bytes from two calls. Measured on MI355X: see DESIGN.md section 6."""
    sl, blank = sc_cases.GRAD_INSTANCE_SL, None if five else sc_cases.BLANK
    raw, ntc, targets, lengths, wt = sc_cases.grad_instance_case(npos, five)
    row = sc_cases.chain_instance(targets.shape[1], sl)
    assert npos <= np.prod(sc_cases.GEOMETRY[row]) and (row == 0 or npos > np.prod(sc_cases.GEOMETRY[row - 1]))
    r64, g32 = _chain_refs(ntc, targets, lengths, sl, five, wt)
    want = r64["grad"]
    assert np.isfinite(r64["logz"]).all()
    x = torch.from_numpy(raw).cuda()
    tg, ln, w = torch.from_numpy(targets), torch.from_numpy(lengths), torch.from_numpy(wt)
    plain = decode.seq_logz(x, tg, ln, sl, blank)
    logz, g = decode.seq_logz_grad(x, tg, ln, sl, blank, weight=w)
    assert torch.equal(logz, plain) and bool(torch.isfinite(logz).all())               # bit for bit the forward scan
    got = _ntc(g, five).astype(np.float64)
    dk = float(np.abs(got - want).max())
    print("npos %d %s %s: g32 %.3e kernel %.3e (share %s)" % (npos, "5S" if five else "koi", sc_cases.GEOMETRY[row], g32, dk, r64["share"].tolist()))
    assert wt[3] == 0.0 and not got[3].any()                                            # the weight-0 row: exactly zero
    assert (np.abs(got - want) <= _chain_bound(r64, g32, wt, want, torch.float16)).all(), (dk, g32)
    if five:                                                                            # a path takes one edge per step
        total = _chain_bound(r64, g32, wt, want, torch.float16).sum(axis=2)              # the per-element bound, summed over the step
        ds = np.abs(got.sum(axis=2) - wt[:, None])
        print("    a step's gradient against the row's weight: %.3e (allowed %.3e .. %.3e)" % (ds.max(), total.min(), total.max()))
        assert (ds <= total).all()
    if npos in sc_cases.GRAD_FIRST_SIZES:
        zero = want == 0
        assert zero.any() and (not zero.all() or (npos == 1 and not five))               # (one position, koi layout: no edge has an element)
        # fp32 output into a NaN-filled tensor; then fp16 with int32 targets
        out = torch.full(x.shape, float("nan"), dtype=torch.float32, device="cuda")
        lz, g2 = decode.seq_logz_grad(x, tg, ln, sl, blank, weight=w, out=out)
        assert g2 is out and torch.equal(lz, plain)
        got32 = _ntc(out, five).astype(np.float64)
        assert np.isfinite(got32).all() and not got32[zero].any() and not got32[3].any()
        d32 = float(np.abs(got32 - want).max())
        assert (np.abs(got32 - want) <= _chain_bound(r64, g32, wt, want, torch.float32)).all(), (d32, g32)
        out = torch.full(x.shape, float("nan"), dtype=torch.float16, device="cuda")
        lz, _ = decode.seq_logz_grad(x, tg.to(torch.int32), ln, sl, blank, weight=w, out=out)
        assert torch.equal(lz, plain) and torch.equal(out, g)                            # int32 rows: the same bits; every element written
        assert not _ntc(out, five)[zero].any()
        worst = 0.0
        for dtype in (torch.float16, torch.float32):
            fill = 3.0
            buf, view, mask = _guarded_out(x.shape, dtype, fill)
            lz, g3 = decode.seq_logz_grad(x, tg, ln, sl, blank, weight=w, out=view, accumulate=True)
            assert g3 is view and torch.equal(lz, plain)
            assert bool((buf[~mask] == fill).all()), "guard elements around the strided gradient were written"
            acc = _ntc(view, five).astype(np.float64)
            assert (acc[zero] == fill).all() and (acc[3] == fill).all()                  # nothing gathered, weight 0: the fill itself
            worst = max(worst, float(np.abs(acc - (want + fill)).max()))
            assert (np.abs(acc - (want + fill)) <= _chain_bound(r64, g32, wt, want + fill, dtype)).all(), (dtype, worst)
        print("    first size: fp32 output %.3e, accumulate %.3e" % (d32, worst))
    if npos in (257, 2049):                                                              # determinism: bit-identical from call to call
        assert torch.equal(g, decode.seq_logz_grad(x, tg, ln, sl, blank, weight=w)[1])
        f32 = torch.zeros(x.shape, dtype=torch.float32, device="cuda")
        a = decode.seq_logz_grad(x, tg, ln, sl, blank, weight=w, out=f32)[1].clone()
        assert torch.equal(a, decode.seq_logz_grad(x, tg, ln, sl, blank, weight=w, out=f32)[1])


@pytest.mark.parametrize("five", [False, True], ids=["koi", "5S"])
@pytest.mark.parametrize("T", sc_cases.GRAD_WIDE_T)
@pytest.mark.parametrize("sl", sc_cases.GRAD_WIDE_SL)
def test_short_rows_in_a_four_wave_launch(sl, T, five):
    """grad_wide_case: rows of k, k + 1, k + (T + 1) // 2 and k + T labels and one that cannot fit, zero-padded to 600 columns: the
    launch takes the 256 x 4 instance, where all but one or a few threads hold no position of the row, most store no alpha, and thread 0
    picks logz. T = 1, 2, 3 lie below the prefetch depth. Both output types, overwrite and accumulate, guard elements."""
    blank = None if five else sc_cases.BLANK
    raw, ntc, targets, lengths, wt = sc_cases.grad_wide_case(sl, T, five)
    row = sc_cases.chain_instance(targets.shape[1], sl)
    assert sc_cases.GEOMETRY[row] == (256, 4) and targets.shape[1] == sc_cases.WIDE       # a four-wave row
    r64, g32 = _chain_refs(ntc, targets, lengths, sl, five, wt)
    fin = np.isfinite(r64["logz"])
    assert fin.tolist() == [True, True, True, True, False] and np.isneginf(r64["logz"][4])
    x = torch.from_numpy(raw).cuda()
    tg = torch.from_numpy(targets).to(torch.int32 if T % 2 else torch.int8)
    ln, w = torch.from_numpy(lengths), torch.from_numpy(wt)
    plain = decode.seq_logz(x, tg, ln, sl, blank)
    assert np.isneginf(plain.cpu().numpy()[4]) and np.isfinite(plain.cpu().numpy()[:4]).all()
    worst = {torch.float16: 0.0, torch.float32: 0.0}
    for dtype in (torch.float16, torch.float32):
        for accumulate in (False, True):
            fill = 3.0
            buf, out, mask = _guarded_out(x.shape, dtype, fill)
            logz, g = decode.seq_logz_grad(x, tg, ln, sl, blank, weight=w, out=out, accumulate=accumulate)
            assert g is out and torch.equal(logz, plain)
            assert bool((buf[~mask] == fill).all()), "guard elements around the strided gradient were written"
            base = fill if accumulate else 0.0
            want = r64["grad"] + base
            got = _ntc(out, five).astype(np.float64)
            assert (got[4] == base).all()                                                # does not fit: nothing added / zeros
            assert (got[r64["grad"] == 0] == base).all()
            worst[dtype] = max(worst[dtype], float(np.abs(got - want).max()))
            assert (np.abs(got - want) <= _chain_bound(r64, g32, wt, want, dtype)).all(), (dtype, accumulate, worst, g32)
    print("wide sl %d T %d %s: g32 %.3e kernel fp32 %.3e fp16 %.3e (share %s)"
          % (sl, T, "5S" if five else "koi", g32, worst[torch.float32], worst[torch.float16], r64["share"].tolist()))


@pytest.mark.parametrize("five", [False, True], ids=["koi", "5S"])
@pytest.mark.parametrize("sl", [1, 2, 3, 4, 5])
def test_dense_gradient_below_the_prefetch_depth(sl, five):
    """T = 1, 2, 3 (below the prefetch depth 4 in both directions) and 5, every state_len - at 1 and 2 the workgroup of 64 threads is
    mostly inactive - N = 3 with weights 1, -0.5, 0: against dense_grad in fp64 within 4 x g32 + the output rounding; the weight-0 row
    exactly zero."""
    blank = None if five else sc_cases.BLANK
    wt = np.array([1.0, -0.5, 0.0])
    C = (5 if five else 4) * 4 ** sl
    for T in sc_cases.TINY_T:
        raw = sc_cases.host_scores((T, 3, C) if five else (3, T, C), 11000 + 100 * sl + 10 * T + five)
        ntc = raw.transpose(1, 0, 2) if five else raw
        _, d64 = gr.dense_grad(ntc, sl, five, blank, weight=wt)
        _, d32 = gr.dense_grad(ntc, sl, five, blank, weight=wt, dtype=np.float32)
        gd32 = float(np.abs(d32.astype(np.float64) - d64).max())
        x = torch.from_numpy(raw).cuda()
        worst = {}
        for xin in (x, x.float()):
            lz, g = decode.logz_grad(xin, sl, blank, weight=torch.from_numpy(wt))
            assert g.dtype == xin.dtype and g.shape == xin.shape
            got = _ntc(g, five).astype(np.float64)
            assert not got[2].any()                                                      # weight 0: exactly zero
            worst[xin.dtype] = float(np.abs(got - d64).max())
            assert (np.abs(got - d64) <= 4 * gd32 + _rounding(d64, xin.dtype)).all(), (T, xin.dtype, worst, gd32)
            assert bool(torch.isfinite(lz).all())
        print("dense sl %d %s T %d: g32 %.3e kernel fp32 %.3e fp16 %.3e" % (sl, "5S" if five else "koi", T, gd32, worst[torch.float32], worst[torch.float16]))


def test_ctc_loss_backward_through_a_four_wave_launch():
    """ctc_loss(...).backward() at state_len 2 on [T = 640, N = 3, 80] scores with targets of 600, 300 and 2 labels: 599 chain positions
    take the 256 x 4 instance, the two-label row is one position inside it. normalise_scores on and off, reduction "mean" and "none"
    with an upstream vector: x.grad against (dense64 - chain64) * w with the bound of test_fixture_ctc_loss_backward; the loss
    bit-equal to the no-grad path."""
    sl, T, N, Lmax = 2, 640, 3, 600
    assert sc_cases.GEOMETRY[sc_cases.chain_instance(Lmax, sl)] == (256, 4)
    raw = sc_cases.host_scores((T, N, 5 * 4 ** sl), 11900)
    ntc = raw.transpose(1, 0, 2)
    lengths = np.array([600, 300, 2], np.int32)
    targets = np.random.default_rng(11901).integers(1, 5, size=(N, Lmax)).astype(np.int8)
    targets[np.arange(Lmax)[None, :] >= lengths[:, None]] = 0
    c64 = gr.chain_grad_banded(ntc, targets, lengths, sl, True)
    c32 = gr.chain_grad_banded(ntc, targets, lengths, sl, True, dtype=np.float32)
    _, d64 = gr.dense_grad(ntc, sl, True)
    _, d32 = gr.dense_grad(ntc, sl, True, dtype=np.float32)
    g32c = float(np.abs(c32["grad"].astype(np.float64) - c64["grad"]).max())
    g32d = float(np.abs(d32.astype(np.float64) - d64).max())
    assert np.isfinite(c64["logz"]).all()
    lens = lengths.astype(np.float64)
    share = c64["share"].astype(np.float64)
    sd = CTC_CRF(sl, ALPHABET)
    base = torch.from_numpy(raw).cuda()
    tg, ln = torch.from_numpy(targets), torch.from_numpy(lengths)
    up = np.array([0.75, -1.25, 2.0])
    for norm in (True, False):
        D = (d64 if norm else 0.0) - c64["grad"]
        mag = (d64 if norm else 0.0) + c64["grad"]
        err = 4 * g32c + (4 * g32d if norm else 0.0) + 2.0 ** -30 * share[:, None, None] + 2.0 ** -22 * mag
        for reduction in ("mean", "none"):
            x = base.clone().requires_grad_(True)
            kw = dict(reduction=reduction, normalise_scores=norm)
            loss = sd.ctc_loss(x, tg, ln, **kw)
            with torch.no_grad():
                assert torch.equal(loss.detach(), sd.ctc_loss(base, tg, ln, **kw))         # bit-equal to the no-grad path
            if reduction == "none":
                loss.backward(torch.from_numpy(up).to(loss))
                w = up / lens
            else:
                loss.backward()
                w = np.full(N, 1.0 / N) / lens
            want = D * w[:, None, None]
            assert x.grad.dtype == torch.float16 and x.grad.shape == x.shape
            got = _ntc(x.grad, True).astype(np.float64)
            bound = err * np.abs(w)[:, None, None] + _rounding(want, torch.float16)
            dk = float(np.abs(got - want).max())
            print("wide ctc_loss norm=%d %s: g32 chain %.3e dense %.3e, backward vs fp64 %.3e" % (norm, reduction, g32c, g32d, dk))
            assert (np.abs(got - want) <= bound).all(), dk

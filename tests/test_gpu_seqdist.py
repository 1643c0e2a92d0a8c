"""CTC-CRF sequence likelihood and forced alignment on the device (-m gpu): bh_crf_seq_logz / bh_crf_seq_viterbi /
bh_crf_seq_logz_free and the Python surface above them against the fp64 restatement (tests/seqdist_ref.py).

TOLERANCE. Nothing is fixed in advance: on the SAME inputs the reference-order fp32 scan (the torch restatement of koi.ctc.logZ_cu run
in fp32 on the CPU) is compared with the fp64 restatement; d32 = the largest absolute distance over the chunks of the case. The kernel
is allowed 4 x d32 (it sums in another order and uses the hardware exp / log). Every test prints both figures; the measured ones are
recorded in DESIGN.md (parity table, "Sequence likelihood"). The edge tests (tests/seqdist_cases.py) add the fp32 spacing of the returned
value, 2e-7 x |want|, since d32 can be zero there; rows without a fixed-start chain take d32 from the fp32 run of sr.free_start_logz.
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import seqdist_cases as sc
import seqdist_ref as sr
from bonito_amd import decode
from bonito_amd.crf.model import CTC_CRF

pytestmark = pytest.mark.gpu

ALPHABET = ["N", "A", "C", "G", "T"]
FIXTURE_CASES = ["sl1_koi", "sl2_koi", "sl3_koi", "sl4_koi", "sl5_koi", "sl1_5s", "sl2_5s", "sl3_5s"]


def _fixture_case(name):
    z = np.load(os.path.join(GOLDEN, "crf_ctc_loss.npz"))
    sl, five = int(name[2]), name.endswith("_5s")
    raw = z[name + "/scores"]
    return z, {"sl": sl, "five": five, "raw": raw, "ntc": raw.transpose(1, 0, 2) if five else raw,
               "blank": None if five else 2.0, "targets": z[name + "/targets"], "lengths": z[name + "/lengths"]}


def _reference_distance(tnc, targets, lengths, sl, five, blank, ref64):
    """d32: how far the reference-order fp32 scan lies from fp64 on these inputs (largest absolute distance, finite entries)."""
    f32 = sr.torch_log_scan_gather(tnc, targets, lengths, sl, five, blank, dtype=torch.float32).numpy().astype(np.float64)
    fin = np.isfinite(ref64)
    assert (np.isneginf(f32) == ~fin).all()
    return float(np.abs(f32[fin] - ref64[fin]).max()) if fin.any() else 0.0


@pytest.mark.parametrize("name", FIXTURE_CASES)
def test_fixture_log_scan_loss_and_alignments(name):
    """Measured on MI355X, per case: reference-order fp32 scan vs fp64 d32 = 2.5e-6 .. 1.4e-5 (sl3_5s the largest), kernel vs fp64 the SAME
    figure to four digits in all eight cases (the kernel evaluates the reference's expression, max + log(1 + exp(min - max)), and the hardware
    exp / log error stays below the fp32 spacing of alpha); dense logZ: fp32 reference dz32 2.0e-5 .. 8.5e-5, kernel 5.0e-6 .. 1.4e-5."""
    z, c = _fixture_case(name)
    sl, five, blank = c["sl"], c["five"], c["blank"]
    x = torch.from_numpy(c["raw"]).cuda()
    tg, ln = torch.from_numpy(c["targets"]), torch.from_numpy(c["lengths"])
    ref64 = sr.log_scan(c["ntc"], c["targets"], c["lengths"], sl, five, blank)
    tnc = torch.from_numpy(c["raw"]) if five else torch.from_numpy(c["raw"]).permute(1, 0, 2)
    d32 = _reference_distance(tnc, c["targets"], c["lengths"], sl, five, blank, ref64)
    fin = np.isfinite(ref64)
    for targets in (tg, tg.to(torch.int32), tg.to(torch.int64)):                      # int8 and int32 rows through the ABI
        got = decode.seq_logz(x, targets, ln, sl, blank).cpu().numpy().astype(np.float64)
        dk = float(np.abs(got[fin] - ref64[fin]).max())
        print("%s: d32 %.3e kernel %.3e" % (name, d32, dk))
        assert (np.isneginf(got) == ~fin).all()                                        # n - 1 > T: -inf exactly
        assert dk <= 4 * d32, (dk, d32)
    # ctc_loss = -(seq_logz - logZ) / len against the fp64 restatement. Its bound is made of the same measured distances: 4 x d32 for the
    # sequence scan plus 4 x dz32 for logZ (dz32: the reference-order fp32 dense scan against fp64 on these scores), over the length, plus
    # the fp32 spacing of the returned loss.
    sd = CTC_CRF(sl, ALPHABET)
    lens = c["lengths"].astype(np.float64)
    lz64 = sr.dense_logz(c["ntc"], sl, five, blank)
    dz32 = float(np.abs(sr.dense_logz(c["ntc"], sl, five, blank, dtype=np.float32).astype(np.float64) - lz64).max())
    lzk = decode.logz_any(x, sl, blank).cpu().numpy()
    print("%s: dz32 %.3e dense logZ kernel %.3e" % (name, dz32, float(np.abs(lzk - lz64).max())))
    assert np.abs(lzk - lz64).max() <= 4 * dz32
    for norm in (True, False):
        loss = sd.ctc_loss(x, tg, ln, reduction="none", normalise_scores=norm, blank_score=blank).cpu().numpy().astype(np.float64)
        want = -(ref64 - (lz64 if norm else 0.0)) / lens
        assert np.isposinf(loss[~fin]).all()
        bound = (4 * d32 + (4 * dz32 if norm else 0.0)) / lens[fin] + 2e-7 * np.abs(want[fin])
        assert (np.abs(loss[fin] - want[fin]) <= bound).all(), (loss, want, bound)
        # ... and the reference's own fp32 numbers from the fixture, which carry one more d32 of their own
        ref = z["%s/loss_%s_none" % (name, "norm" if norm else "raw")].astype(np.float64)
        assert (np.abs(loss[fin] - ref[fin]) <= bound + (d32 + dz32) / lens[fin] + 2e-7 * np.abs(ref[fin])).all()
        mean = float(sd.ctc_loss(x, tg, ln, reduction="mean", normalise_scores=norm, blank_score=blank))
        assert np.isposinf(mean)
    clip = float(z["loss_clip"])
    want = np.clip(-(ref64 - lz64) / lens, 0.0, clip)
    lc = sd.ctc_loss(x, tg, ln, loss_clip=clip, reduction="none", blank_score=blank).cpu().numpy()
    assert np.abs(lc - want).max() <= 4 * (d32 + dz32) + 2e-7 * clip
    assert abs(float(sd.ctc_loss(x, tg, ln, loss_clip=clip, blank_score=blank)) - want.mean()) <= 4 * (d32 + dz32) + 2e-7 * clip
    # Max scan: bit for bit on these fp16-exact cases, tie rule included
    align, best = decode.seq_viterbi(x, tg, ln, sl, blank)
    ra, rb = sr.max_scan(c["ntc"], c["targets"], c["lengths"], sl, five, blank)
    assert (align.numpy() == ra).all() and (align.numpy() == z[name + "/align"]).all()
    assert (best.numpy().astype(np.float64) == rb).all()
    assert (sd.ctc_viterbi_alignments(x, tg, ln, blank_score=blank).numpy() == ra).all()
    if five:
        nrm = sd.normalise(x)
        assert nrm.shape == x.shape and float(decode.logz_any(nrm, sl).abs().max()) < 0.5


def _eighths_case(npos, five):
    """Two chunks at state_len 1 whose rows hold `npos` labels, T = npos + 67 (the traceback crosses an LDS block of 64 steps even at
    npos = 1): row 0 a homopolymer of length npos, row 1 random labels of length max(1, npos - 2), so that its end position is not a
    thread's last slot. Scores are multiples of 1/8 in [-4, 4]: every partial sum of a path is exact in fp32."""
    rng = np.random.default_rng(7000 + npos)
    N, T = 2, npos + 67
    raw = (rng.integers(-32, 33, size=(T, N, 20) if five else (N, T, 16)) / 8).astype(np.float16)
    lengths = np.array([npos, max(1, npos - 2)], np.int32)
    targets = rng.integers(1, 5, size=(N, npos)).astype(np.int8)
    targets[0] = 3
    targets[1, lengths[1]:] = 0
    return raw, (raw.transpose(1, 0, 2) if five else raw), targets, lengths


@pytest.mark.parametrize("five", [False, True])
@pytest.mark.parametrize("npos", [1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096])
def test_max_scan_geometry_every_positions_per_thread(npos, five):
    """Every (threads, positions per thread) instance of the Max scan, at both edges of its range: a call picks its instance by Lmax, so
    the fixtures (small) and the workload size (Lmax 833) reach two of the seven. On multiples of 1/8 the fp32 scan is exact, so the
    kernel returns the alignment and the score of the fp64 restatement, ties included: equality, no tolerance."""
    blank = None if five else 2.0
    raw, ntc, targets, lengths = _eighths_case(npos, five)
    ra, rb = sr.max_scan(ntc, targets, lengths, 1, five, blank)
    assert (ra[:, -1] == lengths - 1).all() and np.isfinite(rb).all()
    align, best = decode.seq_viterbi(torch.from_numpy(raw).cuda(), torch.from_numpy(targets), torch.from_numpy(lengths), 1, blank)
    print("npos %d %s: best %s, %d cells of the alignment differ" % (npos, "5S" if five else "koi", best.numpy(), int((align.numpy() != ra).sum())))
    assert (align.numpy() == ra).all()
    assert (best.numpy().astype(np.float64) == rb).all()


@pytest.mark.parametrize("five", [False, True])
@pytest.mark.parametrize("npos", sc.NPOS)
def test_log_scan_geometry_every_positions_per_thread(npos, five):
    """The plain Log scan against fp64 at both edges of every (threads, positions per thread) instance, on the inputs of the Max-scan sweep
    (state_len 1, T = npos + 67). Measured on MI355X: d32 0 (npos 1: exact) .. 3.4e-3 (npos 4096, koi, |logz| ~ 1.3e3), kernel vs fp64
    the same figure to four digits in 27 of the 28 cases (npos 512 koi: d32 5.2e-5, kernel 7.3e-5)."""
    blank = None if five else 2.0
    raw, ntc, targets, lengths = _eighths_case(npos, five)
    ref64 = sr.log_scan(ntc, targets, lengths, 1, five, blank)
    tnc = torch.from_numpy(raw) if five else torch.from_numpy(raw).permute(1, 0, 2)
    d32 = _reference_distance(tnc, targets, lengths, 1, five, blank, ref64)
    got = decode.seq_logz(torch.from_numpy(raw).cuda(), torch.from_numpy(targets), torch.from_numpy(lengths), 1, blank)
    got = got.cpu().numpy().astype(np.float64)
    dk = float(np.abs(got - ref64).max())
    print("npos %d %s: d32 %.3e kernel %.3e (|logz| ~ %.3g)" % (npos, "5S" if five else "koi", d32, dk, np.abs(ref64).mean()))
    assert np.isfinite(ref64).all() and np.isfinite(got).all()
    assert (np.abs(got - ref64) <= 4 * d32 + 2e-7 * np.abs(ref64)).all(), (got, ref64, d32)


@pytest.mark.parametrize("five", [False, True])
@pytest.mark.parametrize("T", sc.TINY_T)
def test_log_scan_below_the_prefetch_depth(T, five):
    """The plain Log scan at T = 1, 2, 3 and 5 (the ring of four steps ahead is loaded from clamped rows), state_len 3: one chain position,
    two, a move at every step, and one position too many (-inf). Measured on MI355X: d32 0 (T = 1: exact) .. 4.4e-7, kernel 0 .. 4.4e-7
    (|logz| <= 10; in two of the eight cases the kernel lies farther than d32, by 3.2e-8 at the most)."""
    blank = None if five else sc.BLANK
    k = sc.TINY_SL
    raw, ntc, targets, lengths = sc.tiny_log_case(T, five)
    ref64 = sr.log_scan(ntc, targets, lengths, k, five, blank)
    tnc = torch.from_numpy(raw) if five else torch.from_numpy(raw).permute(1, 0, 2)
    d32 = _reference_distance(tnc, targets, lengths, k, five, blank, ref64)
    got = decode.seq_logz(torch.from_numpy(raw).cuda(), torch.from_numpy(targets), torch.from_numpy(lengths), k, blank)
    got = got.cpu().numpy().astype(np.float64)
    fin = np.isfinite(ref64)
    assert fin.tolist() == [True, True, True, False]
    dk = float(np.abs(got[fin] - ref64[fin]).max())
    print("T %d %s: d32 %.3e kernel %.3e, rows %s" % (T, "5S" if five else "koi", d32, dk, got))
    assert (np.isneginf(got) == ~fin).all() and not np.isnan(got).any()
    assert (np.abs(got[fin] - ref64[fin]) <= 4 * d32 + 2e-7 * np.abs(ref64[fin])).all(), (got, ref64, d32)


def _strided(N, T, C, time_major, gen_seed, pad=8, offset=24):
    """Seeded scores in a padded, offset buffer: the view handed to the kernels is neither contiguous nor at the start of its buffer."""
    g = torch.Generator(device="cuda").manual_seed(gen_seed)
    a, b = (T, N) if time_major else (N, T)
    buf = torch.empty(offset + a * b * (C + pad), dtype=torch.float16, device="cuda")
    buf.normal_(0.0, 2.0, generator=g).clamp_(-5, 5)
    return buf[offset:].as_strided((a, b, C), (b * (C + pad), C + pad, 1))


def _targets(N, Lhi, sl, seed):
    rng = np.random.default_rng(seed)
    lengths = np.linspace(sl, Lhi, N).astype(np.int32)
    rng.shuffle(lengths)
    targets = rng.integers(1, 5, size=(N, Lhi)).astype(np.int8)
    targets[np.arange(Lhi)[None, :] >= lengths[:, None]] = 0
    return targets, lengths


@pytest.mark.parametrize("five", [False, True])
@pytest.mark.parametrize("sl", [3, 4, 5])
def test_full_size_log_and_max_scan(sl, five):
    """512 x 1667, target lengths spread from k to T / 2, strided and offset buffers. Measured on MI355X: reference-order
    fp32 scan vs fp64 d32 = 5.8e-3 .. 8.7e-3 (koi layout: 7.4e-3 / 8.7e-3 / 7.9e-3 at state_len 3 / 4 / 5 on |logz| ~ 4.0e3; 5S: 5.8e-3 /
    6.4e-3 / 6.4e-3 on ~ 2.5e3), kernel vs fp64 the same figures to four digits; Max scan: the alignment's fp64 score is the fp64 optimum
    exactly (koi) or within 1.2e-4 (5S), the reported fp32 best within 1.8e-3."""
    N, T, S = 512, 1667, 4 ** sl
    C = (5 if five else 4) * S
    blank = None if five else 2.0
    x = _strided(N, T, C, five, 40 + sl)
    targets, lengths = _targets(N, T // 2, sl, 50 + sl)
    host = x.cpu()
    ntc = host.numpy().transpose(1, 0, 2) if five else host.numpy()
    tnc = host if five else host.permute(1, 0, 2)
    ref64 = sr.log_scan(ntc, targets, lengths, sl, five, blank)
    d32 = _reference_distance(tnc, targets, lengths, sl, five, blank, ref64)
    tg, ln = torch.from_numpy(targets), torch.from_numpy(lengths)
    got = decode.seq_logz(x, tg, ln, sl, blank).cpu().numpy().astype(np.float64)
    dk = float(np.abs(got - ref64).max())
    print("sl %d %s: d32 %.3e kernel %.3e (|logz| ~ %.3g)" % (sl, "5S" if five else "koi", d32, dk, np.abs(ref64).mean()))
    assert np.isfinite(ref64).all() and dk <= 4 * d32, (dk, d32)
    # Max scan: a valid alignment whose fp64 score is the fp64 optimum within the same tolerance; no chunk excluded
    align, best = decode.seq_viterbi(x, tg, ln, sl, blank)
    a = align.numpy()
    assert (a[:, -1] == lengths - sl).all() and (a[:, 0] >= 0).all() and (a[:, 0] <= 1).all()
    steps = np.diff(a, axis=1)
    assert ((steps == 0) | (steps == 1)).all()
    _, opt = sr.max_scan(ntc, targets, lengths, sl, five, blank, traceback=False)
    ps = sr.path_score(ntc, targets, lengths, sl, five, a, blank)
    dv = float(np.abs(ps - opt).max())
    print("sl %d %s: max-scan path score vs fp64 optimum %.3e, reported best vs optimum %.3e"
          % (sl, "5S" if five else "koi", dv, float(np.abs(best.numpy() - opt).max())))
    assert (ps <= opt + 1e-9).all() and dv <= 4 * d32, (dv, d32)
    assert np.abs(best.numpy().astype(np.float64) - ps).max() <= 4 * d32


def _planted_scores(N, T, sl, seed):
    """A k-mer walk with dwell: the true move edge scores +5 at its step, everything else is noise around -2, all within +-5."""
    rng = np.random.default_rng(seed)
    S = 4 ** sl
    sc = np.clip(rng.normal(-2.0, 1.0, size=(N, T, 4 * S)), -5, 5).astype(np.float16)
    for n in range(N):
        state = int(rng.integers(0, S))
        moves = rng.random(T) < 0.4
        for t in np.nonzero(moves)[0]:
            nxt = ((state << 2) | int(rng.integers(0, 4))) & (S - 1)
            sc[n, t, 4 * nxt + state // (S // 4)] = 5.0
            state = nxt
    return sc


def _likelihood_of_calls(scores, sl, name):
    """seq_logprob of the beam search's and the Viterbi decoder's sequences on the HIP path against oracle.crf_ref.seq_logprob."""
    from oracle import crf_ref
    host = scores.cpu().numpy()
    N = host.shape[0]
    bseq, _, _ = decode.beam_search(scores)
    _, vpath = decode.viterbi(scores)
    vseq = decode.path_to_sequence(vpath)
    out = {}
    for label, plane in (("beam", bseq), ("viterbi", vseq)):
        got = decode.seq_logprob(scores, plane).numpy()
        ora = np.array([np.subtract(*crf_ref.seq_logprob(host[i], sl, plane[i].numpy())) for i in range(N)])
        # the Log-scan tolerance on THESE scores and sequences: 4 x (reference-order fp32 scan - fp64) of their fixed-start chains
        tg, ln = decode.encode_sequences(plane)
        ok = ln.numpy() >= sl
        ref64 = sr.log_scan(host[ok], tg.numpy()[ok], ln.numpy()[ok], sl, False, 2.0)
        d32 = _reference_distance(torch.from_numpy(host[ok]).permute(1, 0, 2), tg.numpy()[ok], ln.numpy()[ok], sl, False, 2.0, ref64)
        dk = float(np.abs(got - ora).max())
        print("%s %s: d32 %.3e, seq_logprob vs oracle %.3e (mean ln P %.2f, mean length %.1f)"
              % (name, label, d32, dk, ora.mean(), ln.float().mean()))
        assert np.isfinite(got).all() and dk <= 4 * d32, (label, dk, d32)
        out[label] = got
    wins = int((out["beam"] >= out["viterbi"]).sum())
    print("%s: beam >= Viterbi in ln P(seq | scores) on %d of %d chunks" % (name, wins, N))           # measured, not asserted
    return vseq


@pytest.mark.parametrize("sl", [4, 5])
def test_likelihood_of_called_sequences_planted(sl):
    """Measured on MI355X: d32 8.5e-3 / 8.2e-3, seq_logprob vs the oracle 8.5e-3 / 8.7e-3 (state_len 4 / 5; mean ln P -1.26 / -0.70 at ~ 667
    bases); both decoders call the same sequences here, so beam >= Viterbi on 64 of 64 chunks."""
    scores = torch.from_numpy(_planted_scores(64, 1667, sl, 60 + sl)).cuda()
    _likelihood_of_calls(scores, sl, "planted_sl%d" % sl)


def test_likelihood_of_called_sequences_and_model_loss_hac_random_weights():
    """Measured on MI355X: beam call d32 5.6e-3, vs oracle 6.9e-3 (mean ln P -23.9, 1482 bases); Viterbi call d32 2.2e-2, vs oracle 1.6e-2
    (mean ln P -221.8, 1665 bases); beam >= Viterbi on 64 of 64 chunks; Model.loss mean 0.1245, |loss - restatement| x len <= 2.2e-2."""
    from bonito_amd import synthetic
    from oracle import crf_ref, nn_ref
    model = synthetic.make_model("hac", batchsize=64, chunksize=10000)
    nn_ref.round_params_to_half_(model)
    model.use_koi(batchsize=64, chunksize=10000)
    model = model.half().to("cuda")
    x = torch.randn(64, 1, 10000, generator=torch.Generator().manual_seed(25)).half().cuda()
    scores = model(x)
    sl = model.seqdist.state_len
    assert scores.shape[1] == 1667 and sl == 4
    vseq = _likelihood_of_calls(scores, sl, "hac_random")
    # Model.loss on the engine's own output, with the Viterbi call as the labelled reference: finite, and the restatement's value
    tg, ln = decode.encode_sequences(vseq)
    assert int(ln.min()) >= sl
    loss = model.loss(scores, tg, ln, reduction="none").cpu().numpy().astype(np.float64)
    host = scores.cpu().numpy()
    ref64 = sr.log_scan(host, tg.numpy(), ln.numpy(), sl, False, 2.0)
    d32 = _reference_distance(torch.from_numpy(host).permute(1, 0, 2), tg.numpy(), ln.numpy(), sl, False, 2.0, ref64)
    lz = np.array([crf_ref.seq_logprob(host[i], sl, "", blank=2.0)[1] for i in range(host.shape[0])])
    want = -(ref64 - lz) / ln.numpy()
    print("hac_random Model.loss: mean %.4f, |loss - restatement| * len max %.3e (d32 %.3e)"
          % (loss.mean(), float((np.abs(loss - want) * ln.numpy()).max()), d32))
    assert np.isfinite(loss).all()
    assert (np.abs(loss - want) * ln.numpy() <= 4 * d32 + 2e-7 * np.abs(want) * ln.numpy()).all()
    assert abs(float(model.loss(scores, tg, ln)) - want.mean()) <= 4 * d32
    assert np.allclose(model.seq_logprob(scores, vseq).numpy(), decode.seq_logprob(scores, vseq).numpy())


# ---- the free start (bh_crf_seq_logz_free) at its edges ---------------------------------------------------------------------------------

def _free_rows(host, targets, lengths, sl, dtype):
    """sr.free_start_logz per row of a launch, in `dtype`, as float64."""
    return np.array([sr.free_start_logz(host[n], sc.bases(targets, lengths, n), sl, sc.BLANK, dtype=dtype)
                     for n in range(len(lengths))], np.float64)


def _free_distance(want, w32):
    """d32 of a free-start launch: the fp32 run of the restatement against its fp64 run, largest distance over the finite rows."""
    fin = np.isfinite(want)
    assert (np.isneginf(w32) == ~fin).all() and (np.isneginf(want) == ~fin).all()
    return float(np.abs(w32[fin] - want[fin]).max()) if fin.any() else 0.0


def _assert_free(got, want, d32, tag):
    """Every row of the launch: -inf exactly where the sequence cannot fit, else within 4 x d32 + the fp32 spacing of the value."""
    fin = np.isfinite(want)
    dk = float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0
    print("%s: d32 %.3e kernel %.3e, rows %s" % (tag, d32, dk, got))
    assert not np.isnan(got).any() and (np.isneginf(got) == ~fin).all(), (got, want)
    assert (np.abs(got[fin] - want[fin]) <= 4 * d32 + 2e-7 * np.abs(want[fin])).all(), (tag, got, want, d32)
    return dk


@pytest.mark.parametrize("T", sc.FREE_SHORT_T)
@pytest.mark.parametrize("sl", sc.FREE_STATE_LENS)
def test_free_start_short_lattice_every_state_length(sl, T):
    """One launch holds rows of 0, 1 .. k-1, k, k+1, T-1, T and T+1 labels and a homopolymer, on a padded, offset score view, with int8
    (even T) or int32 (odd T) labels: the closed form of the empty sequence, the finish inside every dense level, the one-position chain
    that only the injection feeds, the sequence that just fits and the one that cannot (-inf); T below the prefetch depth and below k.
    Run twice: in the one-wave instance, and zero-padded to 600 columns, where the same rows go through the 256 x 4 instance and the rows
    the prefix kernel finishes leave the chain kernel early. Measured on MI355X: d32 6.8e-8 (state_len 1, T 1) .. 1.4e-5 (state_len 5, T 24, |logz| <= 65), kernel vs fp64
    6.8e-8 .. 6.9e-6, the same figure in both instances in all 25 cases, at most 1.8 x d32 (state_len 1 T 4, state_len 3 T 5); the
    fixed start of the rows that have a chain: d32 0 .. 7.1e-6, kernel never above it.

    The free start of a sequence does NOT dominate the fixed-start chain of the same row: the chain emits only the labels after its
    first k (20 of 69 such rows of these shapes have free < fixed in fp64). What sums over more paths is the free start of those
    remaining labels - the chain's paths are its paths from one of the 4^k start states - so that is what is asserted, strictly, after
    checking that fp64 separates the two by more than both bounds (measured: by 9.3e-2 at the least, k ln 4 where the chain is one
    position)."""
    targets, lengths = sc.free_short_case(sl, T)
    N = len(lengths)
    x = _strided(N, T, 4 * 4 ** sl, False, 700 + 10 * sl + T)
    host = x.cpu().numpy()
    want = _free_rows(host, targets, lengths, sl, np.float64)
    d32 = _free_distance(want, _free_rows(host, targets, lengths, sl, np.float32))
    assert (np.isfinite(want) == (lengths <= T)).all()
    ln = torch.from_numpy(lengths)
    for tg in (targets, sc.widen(targets)):
        got = decode.seq_logz(x, torch.from_numpy(tg), ln, sl, sc.BLANK, free_start=True).cpu().numpy().astype(np.float64)
        _assert_free(got, want, d32, "sl %d T %d Lmax %d" % (sl, T, tg.shape[1]))
        closed = T * sc.BLANK + sl * np.log(4.0)
        assert lengths[0] == 0 and abs(got[0] - closed) <= 4 * d32 + 2e-7 * closed, (got[0], closed)
    # rows that have a chain: the fixed start against fp64, and the free start of the labels the chain emits strictly above it
    rows = np.nonzero((lengths >= sl) & (lengths <= T))[0]
    if len(rows) == 0:
        assert T < sl
        return
    idx = torch.from_numpy(rows).cuda()
    ftg, fln = targets[rows], lengths[rows]
    f64 = sr.log_scan(host[rows], ftg, fln, sl, False, sc.BLANK)
    df32 = _reference_distance(torch.from_numpy(host[rows]).permute(1, 0, 2), ftg, fln, sl, False, sc.BLANK, f64)
    fixed = decode.seq_logz(x[idx], torch.from_numpy(ftg), torch.from_numpy(fln), sl, sc.BLANK).cpu().numpy().astype(np.float64)
    print("sl %d T %d fixed start: d32 %.3e kernel %.3e" % (sl, T, df32, float(np.abs(fixed - f64).max())))
    assert (np.abs(fixed - f64) <= 4 * df32 + 2e-7 * np.abs(f64)).all(), (fixed, f64, df32)
    stg = np.zeros_like(ftg)
    stg[:, :ftg.shape[1] - sl] = ftg[:, sl:]
    sln = fln - sl
    s64 = _free_rows(host[rows], stg, sln, sl, np.float64)
    ds32 = _free_distance(s64, _free_rows(host[rows], stg, sln, sl, np.float32))
    rest = decode.seq_logz(x[idx], torch.from_numpy(stg), torch.from_numpy(sln), sl, sc.BLANK, free_start=True).cpu().numpy().astype(np.float64)
    _assert_free(rest, s64, ds32, "sl %d T %d labels after the first k" % (sl, T))
    assert (s64 - f64 > 4 * (ds32 + df32) + 2e-7 * (np.abs(s64) + np.abs(f64))).all(), (s64, f64)
    print("sl %d T %d: free start of the emitted labels - fixed start, least %.3e" % (sl, T, float((rest - fixed).min())))
    assert (rest > fixed).all(), (rest, fixed)


@pytest.mark.parametrize("npos", sc.NPOS)
def test_free_start_geometry_every_positions_per_thread(npos):
    """The injected start of the chain kernel at both edges of every (threads, positions per thread) instance, state_len 2 (one real dense
    level in the prefix kernel), against the C oracle in fp64; d32 as for the called sequences: the fixed-start fp32 reference-order scan
    against fp64 on the same scores and rows. The two largest sizes are run twice: same bits. Measured on MI355X: d32 0 (npos 1,
    a one-position chain is exact) .. 2.8e-4 (npos 2048), kernel vs the oracle 4.2e-7 .. 3.3e-4 on |logz| up to 350; closest to the bound
    npos 4096 (3.3e-4 against d32 1.1e-4: 2.9 x) and npos 256 (3.2e-5 against 1.3e-5: 2.4 x). With T = Lmax + 3 a path has three stays
    to place, so at the larger sizes the injection of any single step carries little of the sum: the short lattice above is what pins it."""
    from oracle import crf_ref
    sl = sc.FREE_INSTANCE_SL
    host, targets, lengths = sc.free_instance_case(npos)
    want = np.array([crf_ref.seq_logprob(host[n], sl, sc.text(targets, lengths, n), blank=sc.BLANK)[0] for n in range(3)])
    ref64 = sr.log_scan(host, targets, lengths, sl, False, sc.BLANK)
    d32 = _reference_distance(torch.from_numpy(host).permute(1, 0, 2), targets, lengths, sl, False, sc.BLANK, ref64)
    x, tg, ln = torch.from_numpy(host).cuda(), torch.from_numpy(targets), torch.from_numpy(lengths)
    first = decode.seq_logz(x, tg, ln, sl, sc.BLANK, free_start=True).cpu()
    assert np.isfinite(want).all()
    _assert_free(first.numpy().astype(np.float64), want, d32, "npos %d (|logz| ~ %.3g)" % (npos, np.abs(want).mean()))
    if npos >= 2049:
        again = decode.seq_logz(x, tg, ln, sl, sc.BLANK, free_start=True).cpu()
        assert torch.equal(first.view(torch.int32), again.view(torch.int32))


def test_seq_logprob_short_and_empty_sequences():
    """The surface at state_len 3, T = 24: sequences of 0, 1, 3 (= k) and 10 bases in one call, then every sequence empty - through
    encode_sequences (one padding column) and with targets of no columns at all (the Lmax == 0 branch of the call) - against the C
    oracle's lp - lz. Bound: the free start's, plus 4 x dz32 for the denominator. Measured on MI355X: d32 4.8e-6, dz32 2.4e-5, seq_logprob vs the
    oracle 6.1e-6 (mixed lengths) / 7.5e-6 (all empty)."""
    from oracle import crf_ref
    sl, T, N = 3, 24, 4
    host = sc.host_scores((N, T, 4 * 4 ** sl), 9900)
    x = torch.from_numpy(host).cuda()
    lz64 = sr.dense_logz(host, sl, False, sc.BLANK)
    dz32 = float(np.abs(sr.dense_logz(host, sl, False, sc.BLANK, dtype=np.float32).astype(np.float64) - lz64).max())
    closed = T * sc.BLANK + sl * np.log(4.0)
    for seqs in (["", "A", "ACG", "ACGTACGTAC"], ["", "", "", ""]):
        ora = np.array([crf_ref.seq_logprob(host[n], sl, seqs[n], blank=sc.BLANK) for n in range(N)])
        lp, lz = ora[:, 0], ora[:, 1]
        assert np.abs(lz - lz64).max() < 1e-9 * np.abs(lz).max()
        tg, ln = decode.encode_sequences(seqs)
        w32 = _free_rows(host, tg.numpy(), ln.numpy(), sl, np.float32)
        d32 = _free_distance(lp, w32)
        got = decode.seq_logprob(x, seqs).numpy()
        dk = float(np.abs(got - (lp - lz)).max())
        print("%s: d32 %.3e dz32 %.3e seq_logprob vs oracle %.3e, %s" % (seqs, d32, dz32, dk, got))
        assert np.isfinite(got).all()
        assert (np.abs(got - (lp - lz)) <= 4 * d32 + 2e-7 * np.abs(lp) + 4 * dz32).all(), (got, lp - lz, d32, dz32)
    assert np.abs(lp - closed).max() < 1e-12                                             # (the oracle on the empty sequence)
    assert (np.abs(got - (closed - lz)) <= 4 * d32 + 2e-7 * closed + 4 * dz32).all()
    # no target columns at all: the same numerator, the same bits as through the padding column
    none = decode.seq_logz(x, torch.zeros((N, 0), dtype=torch.int8), torch.zeros(N, dtype=torch.int32), sl, sc.BLANK, free_start=True)
    one = decode.seq_logz(x, tg, ln, sl, sc.BLANK, free_start=True)
    assert (np.abs(none.cpu().numpy().astype(np.float64) - closed) <= 4 * d32 + 2e-7 * closed).all()
    assert torch.equal(none.view(torch.int32), one.view(torch.int32))

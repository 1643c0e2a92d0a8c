"""The CRF decoders plane by plane, instance by instance and traceback block by traceback block against oracle/crf_oracle.c (-m gpu).

tests/test_gpu_decode.py pins the decoders' final outputs; this module pins what lies between: the linear guide b of bs2_backward_kernel
and the planes beta~ / Bcum of crf_backward_kernel to the oracle's BITS, the class posteriors P of every scan instance to the fp64
posteriors within k times the project's own fp32 yardstick, every traceback / staging block boundary, every row of BEAM_INSTANCES (the
BH_BEAM_DEBUG ones included), the search parameters beyond 64 states, independence of a chunk from its neighbours and from what the
workspace held, and the ABI edges. tests/decode_cases.py holds the case lists and the guarded-workspace accessors; the planes are
sliced out of a caller-owned workspace at the offsets the plan hook reports."""
import ctypes as C

import numpy as np
import pytest
import torch

import decode_cases as dc
from bonito_amd import _lib, decode
from conftest import assert_qstrings_agree
from oracle import crf_ref

pytestmark = pytest.mark.gpu


def _assert_beam_equals_oracle(got, want, what):
    seq, qs, mv, qf = got
    oseq, oqs, omv, oqf = want
    assert np.array_equal(mv, omv), what
    assert np.array_equal(seq, oseq), what
    assert np.abs(qf - oqf).max() < 1e-3, what
    assert_qstrings_agree(qs, oqs, oqf)


# ---- A1: the linear guide ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", dc.SCORE_KINDS)
@pytest.mark.parametrize("state_len", dc.STATE_LENS)
def test_guide_rows_equal_the_oracle_bits(state_len, kind):
    """b [N][T+1][S] of bs2_backward_kernel == oracle_bs2_backward, every row 0..T, as bits; every row's maximum lies in [1, 2). The
    search reads only ratios inside a row, so a row rescaled by a wrong power of two (a maximum taken over a neighbouring chunk's lanes)
    changes no sequence until something overflows: only the plane shows it."""
    for i, (N, T) in enumerate(dc.GUIDE_SHAPES[state_len]):
        sc = dc.make_scores(kind, 100 * state_len + i, N, T, state_len)
        for blank in dc.GUIDE_BLANKS:
            want = crf_ref.bs2_backward(sc, state_len, blank=blank)
            for nt in (0, 1):
                with dc.options(decode_nt=nt):
                    run = dc.BeamRun(sc, state_len, blank=blank)
                b = run.guide()
                what = (state_len, kind, N, T, blank, nt)
                assert run.intact(), what
                mx = b.max(axis=2)
                assert (mx >= 1.0).all() and (mx < 2.0).all(), what
                assert np.array_equal(b.view(np.uint32), want.view(np.uint32)), (what, np.argwhere(b.view(np.uint32) != want.view(np.uint32))[:4])


# ---- A2: class posteriors ----------------------------------------------------------------------------------------------------------------
POSTERIOR_PARAMS = [(sl, name) for name, (_, sls) in dc.POSTERIOR_INSTANCES.items() for sl in sls]


@pytest.mark.parametrize("state_len,instance", POSTERIOR_PARAMS)
def test_class_posteriors_within_k_yardsticks_of_fp64(state_len, instance):
    """P [N][T][4] against the fp64 posteriors: dist = max|P - P64| <= k Y, Y = the largest max|P32 - P64| over the state length's cases of
    the project's own fp32 table-lse scan (decode_cases.posterior_yardsticks), k in decode_cases.POSTERIOR_K (chosen from the ratios
    measured on MI355X, DESIGN.md "Decode sweep"). Rows sum to 1 at fp32 level."""
    opts, _ = dc.POSTERIOR_INSTANCES[instance]
    cases, ref, Y = dc.posterior_yardsticks(state_len)
    for case in cases:
        sc, P64, yard = ref[case]
        with dc.options(**opts):
            run = dc.BeamRun(sc, state_len)
        P = run.posteriors()
        assert run.intact(), case
        dist = float(np.abs(P.astype(np.float64) - P64).max())
        print("posterior state_len %d %s %s: Y %.3e yard %.3e dist %.3e ratio %.3f" % (state_len, instance, case, Y, yard, dist, dist / Y))
        assert np.abs(P.astype(np.float64).sum(-1) - 1.0).max() < dc.POSTERIOR_SUM_TOL, case
        assert P.min() >= 0.0
        assert dist <= dc.POSTERIOR_K[state_len] * Y, (case, dist, Y)


# ---- A3: the Log-semiring backward planes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state_len", dc.STATE_LENS)
def test_log_backward_planes_equal_the_oracle_bits(state_len):
    """beta~ [N][T+1][S] and Bcum [N][T+1] of crf_backward_kernel after bh_crf_logz == oracle_crf_backward as bits (same table lse2, same
    order); logZ goes through device libm in double and keeps its tolerance. N = 5 leaves the last workgroup ragged where four or two
    chunks share one; T walks the prefetch ring of four."""
    rng = np.random.default_rng(4000 + state_len)
    for N in dc.BACKWARD_N:
        for T in dc.BACKWARD_T:
            sc = dc.scores(rng, N, T, 4 * dc.n_states(state_len), "normal")
            beta, B, lz = crf_ref.backward(sc, state_len)
            for nt in (0, 1):
                with dc.options(decode_nt=nt):
                    run = dc.LogzRun(sc, state_len)
                what = (state_len, N, T, nt)
                assert run.intact(), what
                assert np.array_equal(run.beta().view(np.uint32), beta.view(np.uint32)), what
                assert np.array_equal(run.bcum().view(np.uint64), B.view(np.uint64)), what
                assert np.allclose(run.logz(), lz, rtol=0, atol=1e-6 * np.abs(lz).max() + 1e-4), what


# ---- B: traceback and staging blocks -------------------------------------------------------------------------------------------------------
def _viterbi_case_scores(sl, five, N, T, kind, seed):
    rng = np.random.default_rng(seed)
    S = dc.n_states(sl)
    if five:
        return dc.scores(rng, T, N, 5 * S, kind)           # [T, N, 5S]
    return dc.scores(rng, N, T, 4 * S, kind)


@pytest.mark.parametrize("kind", ["normal", "ties"])
@pytest.mark.parametrize("case", dc.round1_viterbi_cases(), ids=lambda c: "sl%d-%s-quad%d-N%d-T%d" % (c[0], "5s" if c[1] else "koi", c[2], c[3], c[4]))
def test_viterbi_traceback_blocks(case, kind):
    """Moves, path and best score bit-exact at step counts short of, on, and beyond a traceback block (and two blocks and a step): the
    state carried from one staged block into the next is what these see. Round-1 kernel (state_len 1, 2; 3 with viterbi_quad 0; the 5S
    layout) and the quad kernel."""
    sl, five, quad, N, T = case
    sc = _viterbi_case_scores(sl, five, N, T, kind, 5000 + 97 * sl + T)
    with dc.options(viterbi_quad=quad):
        run = dc.ViterbiRun(sc, sl, layout_5s=five)
    om, op, ob = crf_ref.viterbi(sc, sl, layout_5s=five, blank=2.0, time_major=five)
    mv, path, best = run.outputs()
    assert run.intact()
    assert np.array_equal(path, op), np.argwhere(path != op)[:4]
    assert np.array_equal(mv, om)
    assert np.array_equal(best.view(np.uint32), ob.view(np.uint32))


@pytest.mark.parametrize("case", dc.posterior_viterbi_cases(), ids=lambda c: "sl%d-T%d" % (c[0], c[3]))
def test_posterior_viterbi_traceback_blocks(case):
    """Planted (confident) scores, which the project holds to exact equality with the fp64 oracle, at T = TB, TB + 1 and 2 TB + 1."""
    sl, seed, N, T = case
    sc = dc.make_scores("planted", seed, N, T, sl)
    run = dc.PosteriorViterbiRun(sc, sl)
    om, op = crf_ref.posterior_viterbi(sc, sl)
    mv, path = run.outputs()
    assert run.intact()
    assert np.array_equal(path, op), np.argwhere(path != op)[:4]
    assert np.array_equal(mv, om)


@pytest.mark.parametrize("case", dc.finalize_cases(), ids=lambda c: "sl%d-%s-T%d" % (c[0], c[1], c[4]))
def test_beam_finalize_staging_blocks(case):
    """beam_finalize_kernel stages 256 back-pointer rows a block: T on both sides of one block and beyond two."""
    sl, kind, seed, N, T = case
    sc = dc.make_scores(kind, seed, N, T, sl)
    run = dc.BeamRun(sc, sl)
    assert run.intact()
    _assert_beam_equals_oracle(run.outputs(), crf_ref.beam_search(sc, sl), case)


def test_beam_search_at_the_last_step_tag():
    """T = 2^17 - 1, the largest step count the 17-bit tag of the stay table holds (T = 2^17 is refused: the refusal test)."""
    rng = np.random.default_rng(17)
    sc = dc.peaky_scores(rng, 1, dc.MAX_STEPS, 1)
    run = dc.BeamRun(sc, 1)
    assert run.intact()
    _assert_beam_equals_oracle(run.outputs(), crf_ref.beam_search(sc, 1), "last tag")


# ---- C: the debug instances ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state_len,opts", dc.debug_cases(), ids=lambda v: "fuse%d" % v["beam_fuse"] if isinstance(v, dict) else str(v))
def test_debug_instances_give_the_same_bytes(state_len, opts, monkeypatch):
    """BH_BEAM_DEBUG picks the DBG = true rows of BEAM_INSTANCES (cycle counters into the workspace's debug_counters region): all four
    outputs byte-equal to the plain run, guards intact around a workspace of exactly the exported size. Nothing about the counters."""
    N, T = dc.DEBUG_SHAPE[state_len]
    sc = dc.make_scores("peaky", 6000 + state_len, N, T, state_len)
    with dc.options(**opts):
        monkeypatch.delenv("BH_BEAM_DEBUG", raising=False)
        plain = dc.BeamRun(sc, state_len)
        monkeypatch.setenv("BH_BEAM_DEBUG", "1")
        debug = dc.BeamRun(sc, state_len)
        monkeypatch.delenv("BH_BEAM_DEBUG")
    assert plain.intact() and debug.intact()
    for a, b in zip(plain.outputs(), debug.outputs()):
        assert a.tobytes() == b.tobytes()
    _assert_beam_equals_oracle(debug.outputs(), crf_ref.beam_search(sc, state_len), (state_len, opts))


# ---- D: parameters beyond 64 states ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state_len,opts", dc.param_cases(), ids=lambda v: "-".join("%s%d" % kv for kv in v.items()) or "auto" if isinstance(v, dict) else str(v))
def test_beam_search_parameters(state_len, opts):
    N, T = dc.PARAM_SHAPE[state_len]
    rng = np.random.default_rng(7000 + state_len)
    sc = dc.scores(rng, N, T, 4 * dc.n_states(state_len), "normal")
    for bw in dc.PARAM_WIDTHS:
        for cut, blank in dc.PARAM_CUT_BLANK:
            with dc.options(**opts):
                run = dc.BeamRun(sc, state_len, beam_width=bw, beam_cut=cut, blank=blank, scale=dc.PARAM_SCALE, offset=dc.PARAM_OFFSET)
            want = crf_ref.beam_search(sc, state_len, beam_width=bw, beam_cut=cut, blank=blank, scale=dc.PARAM_SCALE, offset=dc.PARAM_OFFSET)
            assert run.intact()
            _assert_beam_equals_oracle(run.outputs(), want, (state_len, opts, bw, cut, blank))


@pytest.mark.parametrize("kind", ["ties", "zeros"])
@pytest.mark.parametrize("state_len", dc.STATE_LENS)
def test_beam_selection_on_ties_and_zeros(state_len, kind):
    """Many equal keys crowd the boundary bin of the histogram selection (-> its radix fallback); both selections, every state length."""
    N, T = dc.PARAM_SHAPE[state_len]
    rng = np.random.default_rng(8000 + state_len)
    sc = dc.scores(rng, N, T, 4 * dc.n_states(state_len), kind)
    want = crf_ref.beam_search(sc, state_len)
    for select in (0, 1):
        with dc.options(beam_select=select):
            run = dc.BeamRun(sc, state_len)
        assert run.intact()
        _assert_beam_equals_oracle(run.outputs(), want, (state_len, kind, select))


# ---- E: independence and stale memory ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state_len", dc.STATE_LENS)
def test_a_chunk_alone_has_the_bytes_it_has_in_a_batch(state_len):
    """Chunks share waves (below 256 states) and workgroups; a chunk decoded alone gives the bytes it gives between "mixed scale"
    neighbours - beam search (four outputs, and its guide and posterior rows), Viterbi, posterior Viterbi."""
    N, T = (3, 33) if state_len == 5 else (6, 33)
    sc = dc.make_scores("mixed", 9000 + state_len, N, T, state_len)
    sc[N // 2] = dc.make_scores("peaky", 9100 + state_len, 1, T, state_len)[0]         # one chunk that decodes to bases
    beam, vit, pv = dc.BeamRun(sc, state_len), dc.ViterbiRun(sc, state_len), dc.PosteriorViterbiRun(sc, state_len)
    for i in range(N):
        one = sc[i:i + 1]
        b1, v1, p1 = dc.BeamRun(one, state_len), dc.ViterbiRun(one, state_len), dc.PosteriorViterbiRun(one, state_len)
        for whole, alone in zip(beam.outputs() + (beam.guide(), beam.posteriors()), b1.outputs() + (b1.guide(), b1.posteriors())):
            assert whole[i].tobytes() == alone[0].tobytes(), (state_len, i)
        for whole, alone in zip(vit.outputs() + pv.outputs(), v1.outputs() + p1.outputs()):
            assert whole[i].tobytes() == alone[0].tobytes(), (state_len, i)


@pytest.mark.parametrize("state_len", dc.STATE_LENS)
def test_results_do_not_depend_on_what_the_workspace_held(state_len):
    N, T = (2, 21) if state_len == 5 else (5, 37)
    sc = dc.make_scores("peaky", 9500 + state_len, N, T, state_len)
    a, b = dc.BeamRun(sc, state_len, ws_fill=0x00), dc.BeamRun(sc, state_len, ws_fill=0xFF)
    for x, y in zip(a.outputs() + (a.guide(), a.posteriors()), b.outputs() + (b.guide(), b.posteriors())):
        assert x.tobytes() == y.tobytes()
    a, b = dc.LogzRun(sc, state_len, ws_fill=0x00), dc.LogzRun(sc, state_len, ws_fill=0xFF)
    for x, y in zip((a.logz(), a.beta(), a.bcum()), (b.logz(), b.beta(), b.bcum())):
        assert x.tobytes() == y.tobytes()
    a, b = dc.PosteriorViterbiRun(sc, state_len, ws_fill=0x00), dc.PosteriorViterbiRun(sc, state_len, ws_fill=0xFF)
    for x, y in zip(a.outputs(), b.outputs()):
        assert x.tobytes() == y.tobytes()
    assert a.intact() and b.intact()


# ---- F: ABI edges ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state_len", dc.STATE_LENS)
def test_viterbi_stays_inside_its_workspace_and_outputs(state_len):
    """bh_crf_viterbi on exactly bh_crf_viterbi_workspace bytes, guards around the workspace, moves, path and best; both kernels where
    there are two (the quad kernel packs its back-pointers into half the bytes)."""
    N, T = (3, 70) if state_len == 5 else (7, 131)
    rng = np.random.default_rng(9700 + state_len)
    sc = dc.scores(rng, N, T, 4 * dc.n_states(state_len), "ties")
    om, op, ob = crf_ref.viterbi(sc, state_len)
    for quad in ((1, 0) if state_len >= 3 else (1,)):
        with dc.options(viterbi_quad=quad):
            run = dc.ViterbiRun(sc, state_len)
        mv, path, best = run.outputs()
        assert run.intact(), (state_len, quad)
        assert np.array_equal(path, op) and np.array_equal(mv, om) and np.array_equal(best, ob), (state_len, quad)


def _reverse_complement(x, N, T, state_len, five, s_n, s_t, out=None):
    lib = _lib.lib()
    out = torch.full_like(x, 9.0) if out is None else out
    rc = lib.bh_crf_reverse_complement(_lib.ptr(x), _lib.ptr(out), N, T, state_len, int(five), s_n, s_t, _lib.stream_ptr("cuda:0"))
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("five", [False, True], ids=["koi", "5s"])
@pytest.mark.parametrize("state_len", dc.STATE_LENS)
def test_reverse_complement_entry_point(state_len, five):
    """bh_crf_reverse_complement against the index-level restatement, both layouts, dense and with padded rows (row stride 2 C through the
    stride arguments: the padding is neither read nor written); twice is the identity; in == out is refused."""
    N, T = (2, 5) if state_len == 5 else (3, 11)
    S = dc.n_states(state_len)
    Cc = (5 if five else 4) * S
    rng = np.random.default_rng(9800 + state_len)
    sc = dc.scores(rng, T if five else N, N if five else T, Cc, "normal")       # [T, N, 5S] or [N, T, 4S]
    want = crf_ref.reverse_complement(sc, state_len, layout_5s=five)
    x = torch.from_numpy(sc).cuda()
    rows = x.shape[1]
    s_n, s_t = (Cc, N * Cc) if five else (T * Cc, Cc)
    rc, y = _reverse_complement(x, N, T, state_len, five, s_n, s_t)
    assert rc == 0 and np.array_equal(y.cpu().numpy(), want)
    rc, z = _reverse_complement(y, N, T, state_len, five, s_n, s_t)
    assert rc == 0 and torch.equal(z, x)
    padded = torch.full((x.shape[0], rows, 2 * Cc), 7.0, dtype=torch.float16, device="cuda")
    padded[:, :, :Cc] = x
    rc, yp = _reverse_complement(padded, N, T, state_len, five, 2 * s_n, 2 * s_t)
    assert rc == 0 and np.array_equal(yp[:, :, :Cc].cpu().numpy(), want)
    assert bool((yp[:, :, Cc:] == 9.0).all())
    before = x.clone()
    rc, _ = _reverse_complement(x, N, T, state_len, five, s_n, s_t, out=x)
    assert rc != 0 and "in-place" in _lib.last_error() and torch.equal(x, before)


REFUSALS = [
    # (what, N, T, state_len, beam_width, beam_cut, message)
    ("beam_width 0", 2, 9, 2, 0, 100.0, "beam_width"),
    ("beam_width 33", 2, 9, 2, 33, 100.0, "beam_width"),
    ("beam_cut 0.5", 2, 9, 2, 32, 0.5, "beam_cut"),
    ("state_len 0", 2, 9, 0, 32, 100.0, "state_len"),
    ("state_len 6", 2, 9, 6, 32, 100.0, "state_len"),
    ("N 0", 0, 9, 2, 32, 100.0, "empty problem"),
    ("T 2^17", 1, 1 << 17, 1, 32, 100.0, "131071"),
]


@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: c[0].replace(" ", "_"))
def test_beam_search_refusals_launch_nothing(case):
    """A refused call returns non-zero, says why, and writes nothing: outputs and workspace keep their 0xA5 fill. The buffers have the
    size an accepted call of the nearest valid shape would need."""
    what, N, T, sl, bw, cut, message = case
    lib = _lib.lib()
    n_alloc, sl_alloc = max(N, 1), min(max(sl, 1), 5) if sl in (1, 2, 3, 4, 5) else 2
    sc = torch.zeros((n_alloc, T, 4 * dc.n_states(sl_alloc)), dtype=torch.float16, device="cuda")
    ws = dc.Guarded(lib.bh_beam_search_workspace(n_alloc, T, sl_alloc))
    out, qf = dc.Guarded(3 * n_alloc * T), dc.Guarded(4 * n_alloc * T)
    o = out.addr
    rc = lib.bh_beam_search(_lib.ptr(sc), N, T, sl, bw, cut, 2.0, 1.0, 0.0, ws.ptr, C.c_void_p(o), C.c_void_p(o + n_alloc * T),
                            C.c_void_p(o + 2 * n_alloc * T), qf.ptr, _lib.stream_ptr("cuda:0"))
    torch.cuda.synchronize()
    assert rc != 0 and message in _lib.last_error(), (what, _lib.last_error())
    for g in (ws, out, qf):
        assert bool((g.buf == dc.FILL).all()), what

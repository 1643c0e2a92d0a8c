"""The decode sweep of tests/test_gpu_decode_planes.py, checked without a GPU: its case lists reach every kernel instance (through the
plan hook, which touches no device), its bound on the class posteriors would catch a misplaced plane, its step counts sit on the block
constants, and the fp64 oracle agrees with the autograd restatement on the planted posterior-Viterbi seeds the GPU is held to exactly."""
import numpy as np
import pytest

import decode_cases as dc
from bonito_amd import _lib
from oracle import crf_ref


@pytest.fixture()
def set_options():
    handle = _lib.lib()

    def apply(**kw):
        for name, value in kw.items():
            _lib.check(handle.bh_set_option(name.encode(), value), "bh_set_option")
    try:
        yield apply
    finally:
        apply(**dc.OPTION_DEFAULTS)


def test_the_sweep_reaches_every_beam_backward_and_forward_instance(set_options):
    beam, backward, forward = set(), set(), set()
    for sl, N, opts, debug in dc.instance_sweep():
        set_options(**dc.OPTION_DEFAULTS)
        set_options(**opts)
        p = dc.plan(N, 7, sl, debug)
        beam.add(dc.beam_key(p["beam_state_len"], p["beam_cpw"], p["beam_dbg"], p["beam_fuse"]))
        backward.add(p["bwd_state_len"])
        if p["fwd_present"]:
            forward.add(p["fwd_state_len"])
    want = {dc.beam_key(*row) for row in dc.BEAM_INSTANCE_ROWS}
    assert len(want) == 20
    assert beam == want, (sorted(want - beam), sorted(beam - want))
    assert backward == {1, 2, 3, 4, 5} and forward == {1, 2, 3, 4, 5}


def test_every_posterior_instance_is_the_one_its_name_says(set_options):
    for name, (opts, sls) in dc.POSTERIOR_INSTANCES.items():
        for sl in sls:
            set_options(**dc.OPTION_DEFAULTS)
            set_options(**opts)
            p = dc.plan(dc.GUIDE_SHAPES[sl][0][0], 7, sl)
            assert bool(p["beam_fuse"]) == name.startswith("fused") and bool(p["fwd_present"]) == name.startswith("scan_kernel"), (name, sl)
            if name.startswith("fused_cpw"):
                assert p["beam_cpw"] == int(name[-1])
            if name.startswith("scan_kernel_fork"):
                assert p["fwd_on_helper_stream"] == int(name[-1])


def test_step_counts_sit_on_the_block_constants():
    assert [dc.traceback_block(sl) for sl in dc.STATE_LENS] == [512, 512, 512, 128, 32]
    r1 = dc.round1_viterbi_cases()
    assert {t for sl, five, quad, n, t in r1 if sl in (1, 2, 3) and not five and not quad} == {511, 512, 513, 1025}
    assert {(sl, t) for sl, five, quad, n, t in r1 if five} == {(1, 513), (2, 513), (3, 513), (4, 129), (4, 257), (5, 33), (5, 65)}
    assert {(sl, t) for sl, five, quad, n, t in r1 if quad} == {(sl, t) for sl in (3, 4, 5) for t in (63, 64, 65, 129)}
    assert {(sl, t) for sl, _, _, t in dc.posterior_viterbi_cases()} == (
        {(sl, t) for sl in (1, 2, 3) for t in (512, 513, 1025)} | {(4, 128), (4, 129), (4, 257), (5, 32), (5, 33), (5, 65)})
    assert {(sl, t) for sl, kind, _, _, t in dc.finalize_cases() if kind == "peaky"} == {(sl, t) for sl in dc.STATE_LENS for t in (255, 256, 257, 513)}
    assert dc.MAX_STEPS == 131071
    assert set(dc.BACKWARD_T) >= {1, 3, 4, 5} and max(dc.BACKWARD_N) % 4 != 0 and max(dc.BACKWARD_N) % 2 != 0      # SU = 4; ragged last workgroup


@pytest.mark.parametrize("state_len", [1, 2, 3])
def test_mixed_scale_neighbours_rescale_by_different_powers_of_two(state_len):
    """What the "mixed scale" batch is for: below 256 states several chunks share a wave of bs2_backward_kernel, and at EVERY step the
    row maximum of an even chunk has a smaller exponent than that of each odd chunk, so a maximum reduced over a neighbour's lanes
    changes the stored row. One step of the guide recurrence restated in fp64 from the oracle's rows (and held to them)."""
    N, T = dc.GUIDE_SHAPES[state_len][0]
    S = dc.n_states(state_len)
    sc = dc.make_scores("mixed", 100 * state_len, N, T, state_len)            # the GPU test's first case
    b = crf_ref.bs2_backward(sc, state_len).astype(np.float64)
    x = np.clip(sc.astype(np.float64), -40.0, 40.0)
    s = np.arange(S)
    lead = s >> (2 * (state_len - 1))
    expo = np.zeros((N, T), np.int64)
    for t in range(T):
        raw = np.exp(2.0) * b[:, t + 1, :]
        for base in range(4):
            succ = ((s << 2) | base) & (S - 1)
            raw = raw + np.exp(x[:, t, succ * 4 + lead]) * b[:, t + 1, succ]
        expo[:, t] = np.floor(np.log2(raw.max(axis=1)))
        assert np.allclose(raw / 2.0 ** expo[:, t, None], b[:, t, :], rtol=1e-5, atol=0)
    assert (expo[0::2].max(axis=0) < expo[1::2].min(axis=0)).all()


@pytest.mark.parametrize("state_len", dc.STATE_LENS)
def test_posterior_bound_catches_a_misplaced_plane(state_len):
    """P stored one boundary late, and P taken from the neighbouring chunk, both built from the ORACLE's planes, lie beyond ten times the
    bound k Y the kernels are held to; the yardstick itself (the project's fp32 table-lse scan against fp64) stays where it was
    measured when the sweep was written (7e-7 .. 4.1e-5 over random and planted scores), so the bound is tight enough to mean something."""
    cases, ref, Y = dc.posterior_yardsticks(state_len)
    bound = dc.POSTERIOR_K[state_len] * Y
    assert 1e-7 < Y < 1e-4, Y
    assert dc.POSTERIOR_K[state_len] in (2, 4, 8)
    for case in cases:
        sc, P64, yard = ref[case]
        assert yard <= Y
        assert np.abs(P64.astype(np.float64).sum(-1) - 1.0).max() < dc.POSTERIOR_SUM_TOL
        N, T = P64.shape[:2]
        late = np.concatenate([P64[:, :1], P64[:, :-1]], axis=1)
        neighbour = np.roll(P64, 1, axis=0)
        assert np.abs(late - P64).max() > 10 * bound, (case, "late")
        if N > 1:
            assert np.abs(neighbour - P64).max() > 10 * bound, (case, "neighbour")


@pytest.mark.parametrize("state_len", dc.STATE_LENS)
def test_oracle_agrees_with_autograd_on_the_planted_posterior_viterbi_seeds(state_len):
    """The GPU is held to the fp64 oracle EXACTLY on these inputs: that is sound only if the oracle's own path is not a near-tie artefact,
    i.e. the autograd restatement of the reference's decode_batch decodes the same path. The longest case of each state length."""
    sl, seed, N, T = [c for c in dc.posterior_viterbi_cases() if c[0] == state_len][-1]
    assert T == 2 * dc.traceback_block(sl) + 1
    sc = dc.make_scores("planted", seed, N, T, sl)
    moves, path = crf_ref.posterior_viterbi(sc, sl)
    assert np.array_equal(path, crf_ref.posterior_viterbi_autograd(sc, sl))
    assert np.array_equal(moves, (path != 0).astype(np.int8))
    assert 0.2 < moves.mean() < 0.7          # the planted moves are decoded, not an all-blank path

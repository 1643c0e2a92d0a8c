"""The CRF decoders' plane-level sweep (tests/test_gpu_decode_planes.py, checked without a GPU by tests/test_decode_cases_cpu.py): case
lists, score generators, and the accessors that run the C ABI on a guarded workspace and slice the workspace planes out of it.

Every T below is derived from a block constant of the kernels ("Decode sweep", keeps the table):
  crf_viterbi_kernel / crf_posterior_viterbi_kernel   TB = min(512, 32768 / S) back-pointer rows per traceback block
  crf_viterbi_quad_kernel                             TB = 64
  beam_finalize_kernel                                FTB = 256
  crf_backward_kernel                                 SU = 4 (prefetch ring), 4 / 2 / 1 chunks per workgroup by state count
  beam_kernel stay table                              17 tag bits: T < 2^17
Nothing here touches the device at import."""
import ctypes as C

import numpy as np

from test_decode_plan_cpu import PLAN_FIELDS, WS_FIELDS, read_plan

STATE_LENS = (1, 2, 3, 4, 5)
GUARD = 4096
FILL = 0xA5
OPTION_DEFAULTS = {"beam_fuse": -1, "beam_cpw": 0, "beam_fork": -1, "beam_select": 0, "decode_nt": 0, "viterbi_quad": 1}
CUS = 256               # compute units of an MI355X: what bh_cu_count() hands the plan on the device the sweep runs on


def n_states(state_len):
    return 4 ** state_len


def traceback_block(state_len):
    """TB of crf_viterbi_kernel and crf_posterior_viterbi_kernel."""
    return max(1, min(512, 32768 // n_states(state_len)))


QUAD_TB = 64
FINALIZE_TB = 256
MAX_STEPS = (1 << 17) - 1


# ---- score generators -----------------------------------------------------------------------------------------------------------------
def scores(rng, N, T, C_, kind):
    """fp16 [N, T, C] within +-5: "normal", "tanh", "ties" (rounded to integers: many exact ties), "zeros"."""
    if kind == "zeros":
        return np.zeros((N, T, C_), np.float16)
    x = rng.standard_normal((N, T, C_)) * 2.0
    if kind == "tanh":
        x = np.tanh(x) * 5.0
    elif kind == "ties":
        x = np.round(x)
    return np.clip(x, -5, 5).astype(np.float16)


def peaky_scores(rng, N, T, state_len, sharp=3.0):
    """Scores with a planted path so that a decoder emits realistic base runs."""
    S = n_states(state_len)
    x = rng.standard_normal((N, T, 4 * S)).astype(np.float32)
    for n in range(N):
        st = int(rng.integers(S))
        for t in range(T):
            if rng.random() < 0.35:
                b = int(rng.integers(4))
                new = ((st << 2) | b) & (S - 1)
                x[n, t, new * 4 + (st >> (2 * (state_len - 1)))] += 2.0 * sharp
                st = new
            else:
                x[n, t] -= sharp * 0.5
    return np.clip(x, -5, 5).astype(np.float16)


def planted_scores(rng, N, T, state_len):
    """Confident, model-like scores: a background around -3 and one planted move of 4.5 on 45 % of the steps. Posterior decoding of these
    is held to EXACT equality with the fp64 oracle (the edge posteriors have no near-ties)."""
    S = n_states(state_len)
    sc = (rng.standard_normal((N, T, 4 * S)) * 0.5 - 3.0)
    for n in range(N):
        st = int(rng.integers(S))
        for t in range(T):
            if rng.random() < 0.45:
                new = (st * 4 + int(rng.integers(4))) % S
                sc[n, t, new * 4 + st // (S // 4)] = 4.5
                st = new
    return np.clip(sc, -5, 5).astype(np.float16)


def out_of_range_scores(rng, N, T, state_len):
    """Far outside what a trained head emits: N(0, 30), 1 % entries at each end of the fp16 range, chunk 0 all -60000 (every move
    numerically impossible), the first half of chunk 1 all 60000 (every move saturates). Needs N >= 2."""
    S = n_states(state_len)
    sc = (rng.normal(0, 30, (N, T, 4 * S))).astype(np.float16)
    sc[rng.random(sc.shape) < 0.01] = np.float16(65504)
    sc[rng.random(sc.shape) < 0.01] = np.float16(-65504)
    sc[0, :, :] = np.float16(-60000)
    sc[1, : T // 2, :] = np.float16(60000)
    return sc


def mixed_scale_scores(rng, N, T, state_len):
    """Consecutive chunks alternate between all entries near -5 and all near +5: a guide row of an even chunk barely grows (e^2 from the
    stay), a row of an odd chunk grows by ~4 e^5 a step, so chunks that share a wave carry row maxima with different exponents at every
    step. A maximum reduced over the lanes of a neighbour rescales by the wrong power of two."""
    S = n_states(state_len)
    x = rng.standard_normal((N, T, 4 * S)) * 0.25
    x += np.where(np.arange(N) % 2 == 1, 5.0, -5.0)[:, None, None]
    return x.astype(np.float16)


SCORE_KINDS = ("normal", "peaky", "out_of_range", "mixed")


def make_scores(kind, seed, N, T, state_len):
    rng = np.random.default_rng(seed)
    if kind == "peaky":
        return peaky_scores(rng, N, T, state_len)
    if kind == "planted":
        return planted_scores(rng, N, T, state_len)
    if kind == "out_of_range":
        return out_of_range_scores(rng, N, T, state_len)
    if kind == "mixed":
        return mixed_scale_scores(rng, N, T, state_len)
    return scores(rng, N, T, 4 * n_states(state_len), kind)


# ---- A: plane cases ---------------------------------------------------------------------------------------------------------------------
# (N, T) of the guide / posterior sweeps: chunk counts on both sides of what a wave packs (64 / 16 / 4 chunks below 256 states), T short
# of and beyond the staging blocks
GUIDE_SHAPES = {1: [(65, 9), (3, 300)], 2: [(17, 9), (3, 300)], 3: [(5, 9), (3, 300)], 4: [(5, 9), (3, 130)], 5: [(2, 5), (2, 40)]}
GUIDE_BLANKS = (2.0, -30.0, 30.0)
BACKWARD_N = (1, 5)
BACKWARD_T = (1, 3, 4, 5, 9, 130)
POSTERIOR_KINDS = ("normal", "peaky")        # within +-5: clipped normal and planted

# Instances that produce P: name -> (options, state lengths). The stand-alone scan runs with the fork option both ways.
POSTERIOR_INSTANCES = {
    "scan_kernel_fork0": (dict(beam_fuse=0, beam_fork=0), (1, 2, 3, 4, 5)),
    "scan_kernel_fork1": (dict(beam_fuse=0, beam_fork=1), (1, 2, 3, 4, 5)),
    "fused": (dict(beam_fuse=1), (1, 2, 3)),
    "fused_cpw1": (dict(beam_fuse=1, beam_cpw=1), (4,)),
    "fused_cpw2": (dict(beam_fuse=1, beam_cpw=2), (4,)),
    "fused_cpw4": (dict(beam_fuse=1, beam_cpw=4), (4,)),
}
# k of `max|P_kernel - P64| <= k Y`: the smallest of 2, 4, 8 with (measured on MI355X) max dist / Y <= k / 2. DESIGN.md has the table.
POSTERIOR_K = {1: 2, 2: 2, 3: 2, 4: 2, 5: 2}
POSTERIOR_SUM_TOL = 8 * 2.0 ** -24       # |sum_y P - 1|: four products by one reciprocal (1 ulp) of a three-add fp32 sum


def posterior_cases(state_len):
    """(kind, seed, N, T) of the P sweep at one state length."""
    return [(kind, 1000 + 10 * state_len + i, N, T)
            for kind in POSTERIOR_KINDS for i, (N, T) in enumerate(GUIDE_SHAPES[state_len])]


_YARD = {}


def posterior_yardsticks(state_len):
    """-> (cases, {case: (scores, P64, yard)}, Y): yard = max|P32 - P64| of a case, P32 the project's own fp32 table-lse scan
    (crf_ref.forward_post over crf_ref.backward), Y the largest yard of the state length's cases. CPU only, computed once."""
    from oracle import crf_ref
    if state_len not in _YARD:
        ref = {}
        for case in posterior_cases(state_len):
            kind, seed, N, T = case
            sc = make_scores(kind, seed, N, T, state_len)
            beta, B, lz = crf_ref.backward(sc, state_len)
            P32 = crf_ref.forward_post(sc, state_len, beta, B, lz)
            P64 = crf_ref.posteriors_f64(sc, state_len)
            ref[case] = (sc, P64, float(np.abs(P32.astype(np.float64) - P64).max()))
        _YARD[state_len] = (posterior_cases(state_len), ref, max(v[2] for v in ref.values()))
    return _YARD[state_len]


# ---- B: traceback and staging blocks ------------------------------------------------------------------------------------------------------
def round1_viterbi_cases():
    """(state_len, layout_5s, quad, N, T): every T sits at, one short of, one beyond, or two blocks and one beyond TB."""
    rows = []
    for sl in (1, 2, 3):
        tb = traceback_block(sl)
        rows += [(sl, False, 0, 3, t) for t in (tb - 1, tb, tb + 1, 2 * tb + 1)]
    rows += [(sl, True, 0, 3, traceback_block(sl) + 1) for sl in (1, 2, 3)]
    rows += [(4, True, 0, 3, t) for t in (traceback_block(4) + 1, 2 * traceback_block(4) + 1)]
    rows += [(5, True, 0, 1, t) for t in (traceback_block(5) + 1, 2 * traceback_block(5) + 1)]
    for sl in (3, 4, 5):
        rows += [(sl, False, 1, 3 if sl < 5 else 2, t) for t in (QUAD_TB - 1, QUAD_TB, QUAD_TB + 1, 2 * QUAD_TB + 1)]
    return rows


def posterior_viterbi_cases():
    """(state_len, seed, N, T) with T = TB, TB + 1, 2 TB + 1."""
    return [(sl, 2000 + 10 * sl + i, 2, t) for sl in STATE_LENS
            for i, t in enumerate((traceback_block(sl), traceback_block(sl) + 1, 2 * traceback_block(sl) + 1))]


def finalize_cases():
    """(state_len, kind, seed, N, T) around FTB. Peaky scores keep the best element in slot 0 for most of a chunk, and a traceback that
    lost its slot at a block boundary would start the next block from the final slot - often 0 too; clipped-normal scores spread the
    surviving path over the slots."""
    return [(sl, kind, 3000 + 10 * sl + i, 1 if sl == 5 else 2, t) for sl in STATE_LENS for kind in ("peaky", "normal")
            for i, t in enumerate((FINALIZE_TB - 1, FINALIZE_TB, FINALIZE_TB + 1, 2 * FINALIZE_TB + 1))]


# ---- C: every instance ------------------------------------------------------------------------------------------------------------------
def beam_key(state_len, cpw, dbg, fuse):
    """beam_key of csrc/beam.hip."""
    return state_len * 100 + cpw * 10 + (2 if dbg else 0) + (1 if fuse else 0)


# the 20 rows of BEAM_INSTANCES (csrc/beam.hip), as (STATE_LEN, CPW, DBG, FUSE)
BEAM_INSTANCE_ROWS = [
    (4, 4, False, True), (4, 2, False, True),
    (1, 4, False, True), (1, 4, True, True), (2, 4, False, True), (2, 4, True, True), (3, 4, False, True), (3, 4, True, True),
    (4, 1, False, True), (4, 1, True, True),
    (1, 4, False, False), (1, 4, True, False), (2, 4, False, False), (2, 4, True, False), (3, 4, False, False),
    (3, 4, True, False), (4, 1, False, False), (4, 1, True, False), (5, 1, False, False), (5, 1, True, False)]

DEBUG_SHAPE = {1: (5, 33), 2: (5, 33), 3: (5, 33), 4: (5, 33), 5: (2, 17)}


def debug_cases():
    """(state_len, options): fused and unfused where both exist."""
    return [(sl, dict(beam_fuse=f)) for sl in STATE_LENS for f in ((1, 0) if sl <= 4 else (0,))]


def instance_sweep():
    """(state_len, N, options, debug) of every bh_beam_search call of the GPU sweep that picks an instance on purpose: the P sweep and the
    debug runs (each with the plain run it is compared with)."""
    rows = []
    for name, (opts, sls) in POSTERIOR_INSTANCES.items():
        for sl in sls:
            for _, _, N, _ in posterior_cases(sl):
                rows.append((sl, N, opts, 0))
    for sl, opts in debug_cases():
        rows.append((sl, DEBUG_SHAPE[sl][0], opts, 0))
        rows.append((sl, DEBUG_SHAPE[sl][0], opts, 1))
    return rows


# ---- D: parameters ---------------------------------------------------------------------------------------------------------------------
PARAM_WIDTHS = (1, 2, 5, 31, 32)
PARAM_CUT_BLANK = ((1.0, 2.0), (2.0, 0.5), (100.0, 2.0), (1e6, -1.0))
PARAM_SCALE, PARAM_OFFSET = 1.05, 0.2
PARAM_SHAPE = {1: (5, 60), 2: (5, 60), 3: (5, 60), 4: (5, 60), 5: (2, 30)}


def param_cases():
    """(state_len, options) of the parameter sweep: 256 states both fused (four chunks per workgroup) and unfused."""
    return [(1, {}), (2, {}), (4, dict(beam_fuse=1, beam_cpw=4)), (4, dict(beam_fuse=0)), (5, {})]


# ---- accessors (device) ----------------------------------------------------------------------------------------------------------------
class options:
    """with options(beam_fuse=0): ...  - process-wide options set for the block, the defaults put back behind it."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        from bonito_amd import decode
        for k, v in self.kw.items():
            decode.set_option(k, v)

    def __exit__(self, *exc):
        from bonito_amd import decode
        for k in self.kw:
            decode.set_option(k, OPTION_DEFAULTS[k])


def layout(N, T, state_len):
    """Byte offsets of the workspace regions (WS_FIELDS) by the plan hook."""
    from bonito_amd import _lib
    _, lay = read_plan(_lib.lib(), N, T, state_len, CUS, 0)
    return dict(zip(WS_FIELDS, lay))


def plan(N, T, state_len, debug=0, cus=CUS):
    from bonito_amd import _lib
    got, _ = read_plan(_lib.lib(), N, T, state_len, cus, debug)
    return dict(zip(PLAN_FIELDS, got))


class Guarded:
    """`nbytes` of device memory filled with `fill`, with GUARD bytes of 0xA5 on either side."""

    def __init__(self, nbytes, fill=FILL):
        import torch
        self.n = int(nbytes)
        self.buf = torch.full((self.n + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda")
        if fill != FILL:
            self.buf[GUARD:GUARD + self.n] = fill
        self.addr = self.buf.data_ptr() + GUARD
        self.ptr = C.c_void_p(self.addr)

    @property
    def body(self):
        return self.buf[GUARD:GUARD + self.n]

    def intact(self):
        import torch
        torch.cuda.synchronize()
        return bool((self.buf[:GUARD] == FILL).all()) and bool((self.buf[GUARD + self.n:] == FILL).all())

    def view(self, dtype, shape, offset=0):
        """A host copy of `shape` elements of `dtype` at byte `offset` of the body."""
        import torch
        torch.cuda.synchronize()
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return self.body[offset:offset + n].cpu().numpy().view(dtype).reshape(shape).copy()


class BeamRun:
    """One bh_beam_search call on a workspace of exactly bh_beam_search_workspace bytes between guards, outputs between guards too."""

    def __init__(self, sc, state_len, beam_width=32, beam_cut=100.0, blank=2.0, scale=1.0, offset=0.0, ws_fill=FILL, check=True):
        import torch
        from bonito_amd import _lib
        lib = _lib.lib()
        self.N, self.T, self.sl = N, T, state_len = sc.shape[0], sc.shape[1], state_len
        self.dev = sc if isinstance(sc, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(sc)).cuda()
        self.lay = layout(N, T, state_len)
        assert lib.bh_beam_search_workspace(N, T, state_len) == self.lay["beam_total"]
        self.ws = Guarded(self.lay["beam_total"], ws_fill)
        self.out = Guarded(3 * N * T)
        self.qf = Guarded(4 * N * T)
        o = self.out.addr
        self.rc = lib.bh_beam_search(_lib.ptr(self.dev), N, T, state_len, int(beam_width), float(beam_cut), float(blank), float(scale),
                                     float(offset), self.ws.ptr, C.c_void_p(o), C.c_void_p(o + N * T), C.c_void_p(o + 2 * N * T),
                                     self.qf.ptr, _lib.stream_ptr("cuda:0"))
        if check:
            _lib.check(self.rc, "bh_beam_search")
        torch.cuda.synchronize()

    def intact(self):
        return self.ws.intact() and self.out.intact() and self.qf.intact()

    def outputs(self):
        """(sequence, qstring, moves, qfloat) as numpy arrays."""
        planes = self.out.view(np.int8, (3, self.N, self.T))
        return planes[0], planes[1], planes[2], self.qf.view(np.float32, (self.N, self.T))

    def guide(self):
        return self.ws.view(np.float32, (self.N, self.T + 1, n_states(self.sl)), self.lay["beta"])

    def posteriors(self):
        return self.ws.view(np.float32, (self.N, self.T, 4), self.lay["P"])


class LogzRun:
    """One bh_crf_logz call on a guarded workspace of bh_beam_search_workspace bytes: beta~, Bcum and logZ."""

    def __init__(self, sc, state_len, blank=2.0, ws_fill=FILL):
        import torch
        from bonito_amd import _lib
        lib = _lib.lib()
        self.N, self.T, self.sl = N, T, state_len = sc.shape[0], sc.shape[1], state_len
        self.dev = torch.from_numpy(np.ascontiguousarray(sc)).cuda()
        self.lay = layout(N, T, state_len)
        self.ws = Guarded(self.lay["beam_total"], ws_fill)
        self.lz = Guarded(8 * N)
        _lib.check(lib.bh_crf_logz(_lib.ptr(self.dev), N, T, state_len, float(blank), self.ws.ptr, self.lz.ptr, _lib.stream_ptr("cuda:0")),
                   "bh_crf_logz")
        torch.cuda.synchronize()

    def intact(self):
        return self.ws.intact() and self.lz.intact()

    def beta(self):
        return self.ws.view(np.float32, (self.N, self.T + 1, n_states(self.sl)), self.lay["beta"])

    def bcum(self):
        return self.ws.view(np.float64, (self.N, self.T + 1), self.lay["Bcum"])

    def logz(self):
        return self.lz.view(np.float64, (self.N,))


class PosteriorViterbiRun:
    """One bh_crf_posterior_viterbi call on a guarded workspace of exactly bh_crf_posterior_viterbi_workspace bytes."""

    def __init__(self, sc, state_len, blank=2.0, ws_fill=FILL):
        import torch
        from bonito_amd import _lib
        lib = _lib.lib()
        self.N, self.T, self.sl = N, T, state_len = sc.shape[0], sc.shape[1], state_len
        self.dev = torch.from_numpy(np.ascontiguousarray(sc)).cuda()
        self.lay = layout(N, T, state_len)
        assert lib.bh_crf_posterior_viterbi_workspace(N, T, state_len) == self.lay["posterior_viterbi_total"]
        self.ws = Guarded(self.lay["posterior_viterbi_total"], ws_fill)
        self.out = Guarded(2 * N * T)
        o = self.out.addr
        _lib.check(lib.bh_crf_posterior_viterbi(_lib.ptr(self.dev), N, T, state_len, float(blank), self.ws.ptr, C.c_void_p(o),
                                                C.c_void_p(o + N * T), _lib.stream_ptr("cuda:0")), "bh_crf_posterior_viterbi")
        torch.cuda.synchronize()

    def intact(self):
        return self.ws.intact() and self.out.intact()

    def outputs(self):
        """(moves, path)"""
        planes = self.out.view(np.int8, (2, self.N, self.T))
        return planes[0], planes[1]


class ViterbiRun:
    """One bh_crf_viterbi call on exactly bh_crf_viterbi_workspace bytes between guards; moves, path and best each between guards.
    `sc` is [N, T, 4S] (koi layout) or [T, N, 5S] (layout_5s)."""

    def __init__(self, sc, state_len, layout_5s=False, blank=2.0):
        import torch
        from bonito_amd import _lib
        lib = _lib.lib()
        Cc = sc.shape[2]
        if layout_5s:
            T, N = sc.shape[:2]
            s_n, s_t = Cc, N * Cc
        else:
            N, T = sc.shape[:2]
            s_n, s_t = T * Cc, Cc
        self.N, self.T = N, T
        self.dev = torch.from_numpy(np.ascontiguousarray(sc)).cuda()
        self.ws = Guarded(lib.bh_crf_viterbi_workspace(N, T, state_len))
        self.moves, self.path, self.best = Guarded(N * T), Guarded(N * T), Guarded(4 * N)
        _lib.check(lib.bh_crf_viterbi(_lib.ptr(self.dev), N, T, state_len, int(layout_5s), float(blank), s_n, s_t, self.ws.ptr,
                                      self.moves.ptr, self.path.ptr, self.best.ptr, _lib.stream_ptr("cuda:0")), "bh_crf_viterbi")
        torch.cuda.synchronize()

    def intact(self):
        return self.ws.intact() and self.moves.intact() and self.path.intact() and self.best.intact()

    def outputs(self):
        """(moves, path, best)"""
        return (self.moves.view(np.int8, (self.N, self.T)), self.path.view(np.int8, (self.N, self.T)),
                self.best.view(np.float32, (self.N,)))

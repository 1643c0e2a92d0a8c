"""Plain fp64 restatements of the CTC head (1x1 decoder convolution + log_softmax, bh_ctc_head) and of the residual RMSNorm
(bh_rmsnorm_residual), each with the tolerance it allows per element, and the seeded inputs that tests/test_gpu_ctc_kernels.py runs the
kernels on and tests/test_ctc_kernels_ref_cpu.py plants errors in. numpy only on the checked path. The greedy and prefix-beam decoders are
restated by oracle/ctc_ref.py; this module adds their inputs and the q-string check with its boundary distance derived from fp32.

Tolerances (|kernel - fp64| per element):
  head     2^-11 |ref| + 2^-25                 the one fp16 rounding at the store (2^-25: half a subnormal step)
           + 2 F 2^-24 (sum_f |w||x| + |b|)    F fused multiply-adds in fp32 (gamma_F of the class's own logit; the row maximum and the
                                               three subtractions and additions around it spend a few of the second F)
           + HEAD_EXPLOG                       the hardware exponential and logarithm inside log(sum exp(logit - max)), see below
  rmsnorm  2^-11 |ref| + 2^-25                 the store
           + 2^-20 |ref|                       the fp32 sum of squares (16 terms per lane, 6 butterfly steps), the division, rsqrtf and the
                                               two multiplies: a relative error of the row's scale factor

HEAD_EXPLOG. No accuracy figure for v_exp_f32 / v_log_f32 was to hand, so the term is measured: over every head case of the GPU suite, the
largest share of |kernel - fp64| that the two derived terms above do not explain, max(0, |d| - store - dot), on MI355X; the term is four
times that. The measured figures stand in the docstring of tests/test_gpu_ctc_kernels.py."""
import numpy as np

HEAD_EXPLOG = 0.0            # 4 x the measured unexplained deviation (0.0: none on any element of the suite)

HEAD_CLASSES = (1, 2, 5, 8)
HEAD_FEATURES = (8, 16, 256, 1032)
HEAD_ROWS = (1, 255, 256, 257, 600)
NORM_D = (8, 64, 504, 512, 520, 1016, 1024)
NORM_M = (1, 3, 4, 5, 1001)
NORM_ALPHA = (0.0, 1.0, 2.449)
NORM_EPS = (1e-5, 1e-3)
GREEDY_CLASSES = (2, 3, 5, 8)
GREEDY_LENGTHS = (0, 1, 2, 255, 256, 257, 511, 512, 513, 1300)
GREEDY_QPARAMS = ((1.0, 0.0), (0.9356, -0.1721), (2.0, 1.0))
BEAM_PAIRS = ((5, 5), (5, 8), (5, 16), (8, 16), (2, 1), (3, 2))          # (classes, beam_size)
BEAM_THRESHOLDS = (0.0, 1e-3, 0.2, 0.999)
BEAM_LENGTHS = (57, 0, 200, 1, 9)
ALPHABET = "NACGTXYZ"


def log_softmax64(z):
    z = np.asarray(z, dtype=np.float64)
    m = z.max(axis=-1, keepdims=True)
    return z - (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))


# ---- CTC head -------------------------------------------------------------------------------------------------------------------
def head_inputs(classes, F, M, large=False):
    """x fp16 [M][F], w fp32 [classes][F], b fp32 [classes]. Ordinary scale: logits ~ N(0, 1) + bias; `large`: logits with a
    standard deviation of 20, so that some reach +-60 (at M = 600): the subtraction of the row maximum decides the result."""
    rng = np.random.default_rng(1000003 * classes + 1009 * F + M + (7 if large else 0))
    x = rng.standard_normal((M, F)).astype(np.float16)
    w = (rng.standard_normal((classes, F)) * ((20.0 if large else 1.0) / np.sqrt(F))).astype(np.float32)
    b = (rng.standard_normal(classes) * 0.5).astype(np.float32)
    return x, w, b


def ctc_head(x, w, b, explog=None):
    """-> (ref fp64 [M][classes], tol fp64 [M][classes])"""
    assert x.dtype == np.float16 and w.dtype == np.float32 and b.dtype == np.float32
    x64, w64, b64 = x.astype(np.float64), w.astype(np.float64), b.astype(np.float64)
    F = x.shape[1]
    ref = log_softmax64(x64 @ w64.T + b64)
    mag = np.abs(x64) @ np.abs(w64).T + np.abs(b64)
    tol = 2.0 ** -11 * np.abs(ref) + 2.0 ** -25 + 2.0 * F * 2.0 ** -24 * mag + (HEAD_EXPLOG if explog is None else explog)
    return ref, tol


def head_row_sum_tolerance(ref, tol):
    """sum_c exp(out) - 1 when every element is within tol of ref: sum_c exp(ref_c) (exp(tol_c) - 1)."""
    return (np.exp(ref) * np.expm1(tol)).sum(axis=-1)


# ---- RMSNorm --------------------------------------------------------------------------------------------------------------------
def norm_inputs(D, M):
    """a, x fp16 [M][D] and a gain w fp32 [D] with a zero and negative entries. From M = 3 on: row 0 all zeros, row 1 of magnitudes near
    6e4 (the sum of squares leaves fp16, not fp32), row 2 of magnitudes near 1e-2 (mean square ~ 1e-4: eps decides the result)."""
    rng = np.random.default_rng(7919 * D + M)
    a = rng.standard_normal((M, D))
    x = rng.standard_normal((M, D))
    if M >= 3:
        a[0] = x[0] = 0.0
        a[1] = rng.choice([-1.0, 1.0], D) * rng.uniform(5.4e4, 6.3e4, D)
        x[1] = rng.choice([-1.0, 1.0], D) * rng.uniform(5.4e4, 6.3e4, D)
        a[2] *= 1e-2
        x[2] *= 1e-2
    w = rng.standard_normal(D).astype(np.float32)
    w[0], w[1] = 0.0, -1.25
    return a.astype(np.float16), x.astype(np.float16), w


def rmsnorm_residual(a, x, w, alpha, eps):
    """out = z / sqrt(mean(z^2) + eps) * w with z = a + alpha x, or z = a where x is None (`a` already holds the sum).
    alpha and eps as the fp32 values the C entry point receives. -> (ref fp64, tol fp64)"""
    assert a.dtype == np.float16 and w.dtype == np.float32 and (x is None or x.dtype == np.float16)
    z = a.astype(np.float64)
    if x is not None:
        z = z + float(np.float32(alpha)) * x.astype(np.float64)
    ref = z / np.sqrt((z * z).mean(axis=-1, keepdims=True) + float(np.float32(eps))) * w.astype(np.float64)
    tol = 2.0 ** -11 * np.abs(ref) + 2.0 ** -25 + 2.0 ** -20 * np.abs(ref)
    return ref, tol


def within(got, ref, tol):
    """Every element finite and within its tolerance. -> (ok, worst |d| / tol, worst |d|)"""
    got = np.asarray(got, dtype=np.float64)
    d = np.abs(got - ref)
    ok = bool(np.isfinite(got).all() and (d <= tol).all())
    return ok, float((d / tol).max()), float(d.max())


# ---- greedy decode --------------------------------------------------------------------------------------------------------------
def _runs(rng, T, C, boost=4.0):
    """[T][C] logits whose argmax comes in runs, some much longer than a thread's segment of ceil(T / 256) steps."""
    labels = np.zeros(T, np.int64)
    t = 0
    while t < T:
        n = int(rng.choice([1, 1, 2, 3, 5, 9, 40, 300]))
        labels[t:t + n] = rng.integers(0, C)
        t += n
    z = rng.standard_normal((T, C))
    z[np.arange(T), labels] += boost
    return z


def greedy_reads(C, R=70):
    """R reads of [T][C] fp32 log-probabilities, T cycling through GREEDY_LENGTHS, the first six planted:
      0  T = 513, its last run (label 1, two steps at p = 0.55) reaches its last step
      1  T = 257, starts with label 1 at p ~ 1 for ONE step: read 0's mean must stop at its end, and read 1 emits again at step 0
      2  T = 512, one label throughout
      3  T = 256, blanks only
      4  T = 255, small-integer logits: exact ties (lowest label wins) and all-equal rows (blank)
      5  T = 511, one-hot rows with p = 1 (every other entry -inf; error clamped to 1e-4) and rows with single -inf entries"""
    rng = np.random.default_rng(4242 + C)
    reads = []
    for i in range(R):
        T = (513, 257, 512, 256, 255, 511)[i] if i < 6 else GREEDY_LENGTHS[i % len(GREEDY_LENGTHS)]
        z = _runs(rng, T, C)
        if i == 0:
            z[-3] = 0.0
            z[-3, 0] = 6.0                       # a blank in front of the last run
            z[-2:] = 0.0
            z[-2:, 1] = np.log(C - 1.0) + 0.2    # p(label 1) = 0.55
        elif i == 1:
            z[0] = 0.0
            z[0, 1] = 12.0
            z[1] = 0.0
            z[1, 0] = 12.0
        elif i == 2:
            z = rng.standard_normal((T, C)) * 0.5
            z[:, C - 1] += 5.0
        elif i == 3:
            z = rng.standard_normal((T, C)) * 0.5
            z[:, 0] += 5.0
        elif i == 4:
            z = np.repeat(rng.integers(0, 3, (T, C)).astype(np.float64), rng.integers(1, 4, T), axis=0)[:T]
            z[::17] = 1.0
        lp = log_softmax64(z).astype(np.float32)
        if i == 5:
            hot = rng.random(T) < 0.4
            lab = np.repeat(rng.integers(0, C, T), rng.integers(1, 6, T))[:T]
            lp[hot] = -np.inf
            lp[hot, lab[hot]] = 0.0
            cold = np.flatnonzero(~hot)
            lp[cold, rng.integers(0, C, cold.size)] = -np.inf
        reads.append(lp)
    return reads


def greedy_q_tolerance(oqf, qscale, qbias):
    """How far from a rounding boundary the oracle's unrounded q may sit where the kernel's character differs. The clamped error
    e = max(1 - p, 1e-4) is recovered from q = -10 log10(e) qscale + qbias. The kernel's e differs by at most 3 * 2^-23 in absolute
    terms (hardware exponential of each step at 2^-23 relative, the mean rounded to fp32, 1 - p rounded), which moves q by
    (10 / ln 10) qscale 3 * 2^-23 / e; q itself is fp32 on both sides: log10f within 2 ulp against numpy's within 1, two multiplies and one
    addition each side, 7 * 2^-24 |q - qbias| + 2 * 2^-24 |q|."""
    q = np.asarray(oqf, dtype=np.float64)
    e = 10.0 ** (-(q - qbias) / (10.0 * qscale))
    return (10.0 / np.log(10.0)) * qscale * 3.0 * 2.0 ** -23 / e + 7.0 * 2.0 ** -24 * np.abs(q - qbias) + 2.0 * 2.0 ** -24 * np.abs(q)


def assert_greedy_qstrings(qs, oqs, oqf, qscale, qbias):
    """The kernel's q-string against the oracle's: a character may differ only where the oracle's unrounded q sits within the derived
    distance of a rounding boundary, then by one, and rarely (conftest.assert_qstrings_agree)."""
    from conftest import assert_qstrings_agree
    qs = np.frombuffer(qs.encode("latin-1"), dtype=np.uint8) if isinstance(qs, str) else np.asarray(qs).astype(np.uint8)
    oqs = np.frombuffer(oqs.encode("latin-1"), dtype=np.uint8) if isinstance(oqs, str) else np.asarray(oqs).astype(np.uint8)
    oqf = np.asarray(oqf, dtype=np.float32)
    assert len(qs) == len(oqs) == len(oqf)
    if len(qs) == 0:
        return 0
    tol = greedy_q_tolerance(oqf, qscale, qbias)
    diff = qs != oqs
    if diff.any():
        frac = (oqf[diff].astype(np.float64) + 0.5) % 1.0
        assert (np.minimum(frac, 1.0 - frac) < tol[diff]).all(), "a q-string byte differs away from a rounding boundary"
    assert_qstrings_agree(qs, oqs, oqf, tol=float(tol[diff].max()) if diff.any() else 0.0)
    return int(diff.sum())


# ---- prefix beam ----------------------------------------------------------------------------------------------------------------
def beam_lanes(C, B):
    """Lanes (reads) per workgroup the launcher picks: the largest of 64, 32, 16, ... whose LDS, 24 B (C + 1) bytes per lane, fits 60 KiB."""
    per_lane = B * C * 24 + B * 24
    L = 64
    while L > 1 and L * per_lane > 60 * 1024:
        L >>= 1
    return L


def beam_reads(C, n, flat=False, T=None):
    """n reads of [T][C] fp32 log-probabilities, T cycling through BEAM_LENGTHS, sharpness through three scales. Read 4 (T = 9) carries
    at step 4 a row whose blank is -inf and whose labels all sit at p = 1e-4: under every threshold above that the beam empties there.
    `flat`: the worst fill, T steps each, for threshold 0 (every label is a candidate). Three reads in four have near-flat rows
    (logits of standard deviation 0.05, 0.5, 1: the candidates barely differ, and the candidate arrays reach B * C entries); every
    fourth has forking rows: two labels at p ~ 1/2 that the step before did not offer, blank and the rest at e^-12, so that from the
    fifth step on ALL B survivors are new prefixes and the node pool grows by B nodes per step, its bound (beam_fill counts both)."""
    assert not flat or C >= 5
    rng = np.random.default_rng(977 * C + (1 if flat else 0))
    reads = []
    for i in range(n):
        if flat and i % 4 == 0:
            z = np.full((T, C), -12.0) + rng.standard_normal((T, C)) * 0.3
            for t in range(T):
                k = 2 * (t % ((C - 1) // 2))
                z[t, 1 + k] += 12.0
                z[t, 2 + k] += 12.0
            lp = log_softmax64(z).astype(np.float32)
        elif flat:
            lp = log_softmax64(rng.standard_normal((T, C)) * (0.05, 0.5, 1.0)[i % 4 - 1]).astype(np.float32)
        else:
            lp = log_softmax64(rng.standard_normal((BEAM_LENGTHS[i % 5], C)) * (0.5, 2.0, 4.0)[i % 3]).astype(np.float32)
            if i == 4:
                lp[4, 0] = -np.inf
                lp[4, 1:] = np.float32(np.log(1e-4))
        reads.append(lp)
    return reads


def beam_fill(lp, B, thr):
    """How full one read drives the prefix beam's arrays: (the most candidates any step holds, nodes allocated). A plain restatement
    of the PB-1 search (oracle/crf_oracle.c::oracle_ctc_prefix_beam) with fp64 logaddexp in place of the table, so the counts are those of
    the same search up to decisions between near-equal scores. The kernel holds B * C candidates and 1 + T * B nodes per read."""
    lp = np.asarray(lp, dtype=np.float64)
    T, C = lp.shape
    lthr = np.log(thr) if thr > 0 else -np.inf
    parent, label, child = [-1], [0], [{}]
    beam = [(0, 0.0, -np.inf)]
    most = 0
    for t in range(T):
        row, cand = lp[t], {}
        for n, pb, pnb in beam:
            tot = np.logaddexp(pb, pnb)
            own = cand.setdefault(n, [-np.inf, -np.inf])
            own[0] = np.logaddexp(own[0], tot + row[0])
            for c in range(1, C):
                if not row[c] >= lthr:
                    continue
                contrib = tot + row[c]
                if n != 0 and label[n] == c:
                    own = cand.setdefault(n, [-np.inf, -np.inf])
                    own[1] = np.logaddexp(own[1], pnb + row[c])
                    contrib = pb + row[c]
                ch = child[n].get(c, -1)
                ext = cand.setdefault(ch if ch >= 0 else -(n * 8 + c) - 1, [-np.inf, -np.inf])
                ext[1] = np.logaddexp(ext[1], contrib)
        most = max(most, len(cand))
        beam = []
        for key, (pb, pnb) in sorted(cand.items(), key=lambda kv: -np.logaddexp(kv[1][0], kv[1][1]))[:B]:
            if np.logaddexp(pb, pnb) == -np.inf:
                continue
            node = key
            if key < 0:
                pn, c = divmod(-(key + 1), 8)
                node = len(parent)
                parent.append(pn), label.append(c), child.append({})
                child[pn][c] = node
            beam.append((node, pb, pnb))
        if beam:
            shift = np.logaddexp(beam[0][1], beam[0][2])
            beam = [(n, pb - shift, pnb - shift) for n, pb, pnb in beam]
    return most, len(parent)

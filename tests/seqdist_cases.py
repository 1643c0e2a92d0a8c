"""Case builders of the sequence-likelihood edge tests, TEST INFRASTRUCTURE ONLY and numpy only: tests/test_gpu_seqdist.py runs these
cases on the device, tests/test_seqdist_cpu.py proves without one that they hold every row class and reach every kernel instance.

* ``free_short_case``: the free start (bh_crf_seq_logz_free) on a short lattice - rows of 0, 1 .. k-1 (finished inside the dense
  levels by seq_prefix_kernel), k (one chain position, fed by the injection only), k + 1, T - 1, T (just fits) and T + 1 (-inf)
  labels, plus a homopolymer; ``widen`` pads the same rows with zero columns so that the launch takes a four-wave instance.
* ``free_instance_case``: the free start at state_len 2 with `npos` chain positions, both edges of every instance row.
* ``tiny_log_case``: the plain Log scan at T below the prefetch depth, lengths k, k + 1, k + T (a move at every step), k + T + 1.
* ``grad_instance_case``: the chain gradient at state_len 2 with `npos` chain positions, either layout, per-row weights; next to the
  full-length rows of free_instance_case it holds a row of k and one of k + 1 labels, which run in whatever instance Lmax selects.
* ``grad_wide_case``: the chain gradient's short rows (k, k + 1, half way, a move at every step, cannot fit) widened to four waves.
* ``chain_instance``: the row of the (threads, positions per thread) list a launch selects - the arithmetic of csrc/seq_chain.h."""
import numpy as np

BLANK = 2.0
FREE_STATE_LENS = (1, 2, 3, 4, 5)
FREE_SHORT_T = (1, 3, 4, 5, 24)
WIDE = 600                                                                    # columns of the widened launch: 596 .. 600 positions
NPOS = (1, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096)    # both edges of every instance row
FREE_INSTANCE_SL = 2
TINY_T = (1, 2, 3, 5)
TINY_SL = 3
GRAD_INSTANCE_SL = 2
GRAD_INSTANCE_WEIGHTS = (1.0, -1.0, 0.5, 0.0, 2.0)
GRAD_FIRST_SIZES = (1, 65, 129, 257, 513, 1025, 2049)                         # the first size of each instance row
GRAD_WIDE_SL = (1, 3, 5)
GRAD_WIDE_T = (1, 2, 3, 5, 24)
GRAD_WIDE_WEIGHTS = (1.0, -1.0, 0.5, 2.0, -0.25)

# (threads, positions per thread) of BH_SEQ_INSTANCES, in its order
GEOMETRY = ((64, 1), (64, 2), (64, 4), (64, 8), (256, 4), (256, 8), (256, 16))


def chain_instance(Lmax, k):
    """The first row that holds max(1, Lmax + 1 - k) positions, -1 beyond the last (chain_instance of csrc/seq_chain.h)."""
    pm = max(1, Lmax + 1 - k)
    for i, (threads, per) in enumerate(GEOMETRY):
        if pm <= threads * per:
            return i
    return -1


def host_scores(shape, seed):
    """fp16 scores as the engine's head gives them: normal(0, 2) clipped to +-5."""
    rng = np.random.default_rng(seed)
    return np.clip(rng.normal(0.0, 2.0, size=shape), -5, 5).astype(np.float16)


def free_short_lengths(sl, T):
    """0, 1 .. k-1, k, k+1, T-1, T, T+1: deduplicated, clipped at 0, ascending."""
    return sorted({max(0, v) for v in list(range(sl + 2)) + [T - 1, T, T + 1]})


def free_short_case(sl, T):
    """(targets [N, Lmax], lengths int32 [N]): one row per length of free_short_lengths with random bases, then a homopolymer of
    min(k + 1, T) labels; Lmax = the longest length; int8 labels for even T, int32 for odd T; 0 = padding."""
    rng = np.random.default_rng(9000 + 100 * sl + T)
    lens = free_short_lengths(sl, T) + [min(sl + 1, T)]
    lengths = np.array(lens, np.int32)
    targets = rng.integers(1, 5, size=(len(lens), max(lens))).astype(np.int32 if T % 2 else np.int8)
    targets[-1] = 2
    targets[np.arange(targets.shape[1])[None, :] >= lengths[:, None]] = 0
    return targets, lengths


def widen(targets, cols=WIDE):
    """The same rows zero-padded to `cols` columns."""
    out = np.zeros((targets.shape[0], cols), targets.dtype)
    out[:, :targets.shape[1]] = targets
    return out


def free_instance_case(npos):
    """(scores fp16 [3, T, 64], targets int8 [3, Lmax], lengths) at state_len 2: Lmax = npos + 1 labels make npos chain positions,
    T = Lmax + 3; a homopolymer of Lmax, random labels of Lmax, and random labels of max(2, Lmax - 2), whose end position is not a
    thread's last slot."""
    rng = np.random.default_rng(9500 + npos)
    Lmax = npos + 1
    T = Lmax + 3
    lengths = np.array([Lmax, Lmax, max(2, Lmax - 2)], np.int32)
    targets = rng.integers(1, 5, size=(3, Lmax)).astype(np.int8)
    targets[0] = 3
    targets[2, lengths[2]:] = 0
    return host_scores((3, T, 4 * 4 ** FREE_INSTANCE_SL), 9600 + npos), targets, lengths


def tiny_log_case(T, five):
    """(raw, scores indexed [n, t, c], targets int8 [4, k + T + 1], lengths) at state_len 3: lengths k, k + 1, k + T and k + T + 1 (-inf);
    raw is [T, 4, 5S] for the reference layout and [4, T, 4S] for the koi layout."""
    k, S = TINY_SL, 4 ** TINY_SL
    rng = np.random.default_rng(9700 + 10 * T + five)
    lengths = np.array([k, k + 1, k + T, k + T + 1], np.int32)
    targets = rng.integers(1, 5, size=(4, k + T + 1)).astype(np.int8)
    targets[np.arange(targets.shape[1])[None, :] >= lengths[:, None]] = 0
    raw = host_scores((T, 4, 5 * S) if five else (4, T, 4 * S), 9800 + 10 * T + five)
    return raw, (raw.transpose(1, 0, 2) if five else raw), targets, lengths


def grad_instance_case(npos, five):
    """(raw, scores indexed [n, t, c], targets int8 [5, Lmax], lengths, weights float64 [5]) at state_len 2: Lmax = npos + 1 and
    T = Lmax + 3 as in free_instance_case; a homopolymer of Lmax, random labels of Lmax, random labels of max(2, Lmax - 2), a row of
    exactly k labels (one chain position) and one of k + 1 (of k where Lmax = k: one position overall). raw is [T, 5, 80] for the
    reference layout and [5, T, 64] (with blank = BLANK) for the koi layout; every row fits."""
    k = GRAD_INSTANCE_SL
    rng = np.random.default_rng(9900 + 2 * npos + five)
    Lmax = npos + 1
    T = Lmax + 3
    lengths = np.array([Lmax, Lmax, max(2, Lmax - 2), k, min(k + 1, Lmax)], np.int32)
    targets = rng.integers(1, 5, size=(5, Lmax)).astype(np.int8)
    targets[0] = 3
    targets[np.arange(Lmax)[None, :] >= lengths[:, None]] = 0
    raw = host_scores((T, 5, 5 * 4 ** k) if five else (5, T, 4 * 4 ** k), 10000 + 2 * npos + five)
    return raw, (raw.transpose(1, 0, 2) if five else raw), targets, lengths, np.array(GRAD_INSTANCE_WEIGHTS)


def grad_wide_case(sl, T, five):
    """(raw, scores indexed [n, t, c], targets int8 [5, WIDE], lengths, weights float64 [5]): rows of k, k + 1, k + (T + 1) // 2 and
    k + T labels (a move at every step; a homopolymer) and one of k + T + 1, which cannot fit, zero-padded to WIDE columns so that the
    launch takes the 256 x 4 instance and almost every thread holds no position of any row."""
    rng = np.random.default_rng(10500 + 100 * sl + 10 * T + five)
    lengths = np.array([sl, sl + 1, sl + (T + 1) // 2, sl + T, sl + T + 1], np.int32)
    targets = rng.integers(1, 5, size=(5, sl + T + 1)).astype(np.int8)
    targets[3] = targets[3, 0]
    targets[np.arange(targets.shape[1])[None, :] >= lengths[:, None]] = 0
    S = 4 ** sl
    raw = host_scores((T, 5, 5 * S) if five else (5, T, 4 * S), 10600 + 100 * sl + 10 * T + five)
    return raw, (raw.transpose(1, 0, 2) if five else raw), widen(targets), lengths, np.array(GRAD_WIDE_WEIGHTS)


def bases(targets, lengths, n):
    """Row n as base indices 0..3."""
    return targets[n, :lengths[n]].astype(np.int64) - 1


def text(targets, lengths, n):
    return "".join("ACGT"[b] for b in bases(targets, lengths, n))

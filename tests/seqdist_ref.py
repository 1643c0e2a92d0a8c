"""Test-side restatements of the CTC-CRF sequence scans (bonito_amd/csrc/seqdist.hip), TEST INFRASTRUCTURE ONLY.

* ``edge_indices`` / ``log_scan`` / ``max_scan``: numpy, any float dtype (fp64 is the yardstick), batched over chunks, gathering the
  stay / move edges from the score rows step by step. The Max scan carries the tie rule of the kernel (a cell is entered by its move
  edge only when that candidate is STRICTLY greater: ties stay) and the same traceback, so alignments compare bit for bit.
* ``torch_logz_cu`` / ``torch_viterbi_alignments``: the torch restatement of koi.ctc.logZ_cu / viterbi_alignments on the
  [T, N, L] stay / move tensors of CTC_CRF.prepare_ctc_scores - the reference-order scan. tests/golden/make_golden_seqdist.py binds
  them to the reference's own class; run in fp32 they are the "reference-order fp32 scan" the GPU tolerance is measured from.
  ``torch_log_scan_gather`` is the same recurrence with the gather done per step (full-size inputs do not fit as [T, N, L]).
* ``enumerate_alignments``: brute force over every monotone alignment (T <= 8).
* ``free_start_logz``: sum over every alignment AND start state, on the full (emitted, state) lattice, any float dtype.

Layouts: ``scores`` is always indexed [n, t, c] here (pass ``x.transpose(1, 0, 2)`` views of [T, N, C] tensors)."""
import itertools

import numpy as np


def edge_indices(targets, state_len, layout_5s):
    """targets [N, Lmax] labels 1..4 (0 = padding) -> (stay_idx [N, n], move_idx [N, n-1]) into a score row, n = Lmax + 1 - k;
    stay_idx is None for the koi layout (the stay score is the scalar blank). move_idx[:, j] scores the edge j -> j + 1."""
    t0 = np.clip(np.asarray(targets).astype(np.int64) - 1, 0, None)
    k = state_len
    n = t0.shape[1] + 1 - k
    kmer = sum(t0[:, i:n + i] * 4 ** (k - i - 1) for i in range(k))
    if layout_5s:
        return kmer * 5, kmer[:, 1:] * 5 + 1 + t0[:, :n - 1]
    return None, kmer[:, 1:] * 4 + t0[:, :n - 1]


def _edges_at(scores, t, stay_idx, move_idx, blank, dtype):
    row = np.asarray(scores[:, t, :])                                         # gather first, widen after: rows are up to 5120 wide
    move = np.take_along_axis(row, move_idx, axis=1).astype(dtype) if move_idx.shape[1] else np.zeros((row.shape[0], 0), dtype)
    stay = np.take_along_axis(row, stay_idx, axis=1).astype(dtype) if stay_idx is not None else dtype(blank)
    return stay, move


def log_scan(scores, targets, lengths, state_len, layout_5s, blank=None, dtype=np.float64):
    """alpha_T[n_i - 1] per chunk, Log semiring; -inf where the chain cannot be walked in T steps."""
    stay_idx, move_idx = edge_indices(targets, state_len, layout_5s)
    N, T = scores.shape[0], scores.shape[1]
    n = move_idx.shape[1] + 1
    alpha = np.full((N, n), -np.inf, dtype)
    alpha[:, 0] = 0
    with np.errstate(invalid="ignore"):
        for t in range(T):
            stay, move = _edges_at(scores, t, stay_idx, move_idx, blank, dtype)
            inc = np.concatenate([np.full((N, 1), -np.inf, dtype), alpha[:, :-1] + move], axis=1)
            alpha = np.logaddexp(alpha + stay, inc).astype(dtype)
    last = np.asarray(lengths).astype(np.int64) - state_len
    return alpha[np.arange(N), last]


def max_scan(scores, targets, lengths, state_len, layout_5s, blank=None, dtype=np.float64, traceback=True):
    """(align int32 [N, T] or None, best [N]): Max semiring, ties stay; rows that cannot be walked are -1 / -inf."""
    stay_idx, move_idx = edge_indices(targets, state_len, layout_5s)
    N, T = scores.shape[0], scores.shape[1]
    n = move_idx.shape[1] + 1
    alpha = np.full((N, n), -np.inf, dtype)
    alpha[:, 0] = 0
    moved = np.zeros((T, N, n), bool) if traceback else None
    for t in range(T):
        stay, move = _edges_at(scores, t, stay_idx, move_idx, blank, dtype)
        inc = np.concatenate([np.full((N, 1), -np.inf, dtype), alpha[:, :-1] + move], axis=1)
        st = alpha + stay
        m = inc > st
        alpha = np.where(m, inc, st).astype(dtype)
        if traceback:
            moved[t] = m
    last = np.asarray(lengths).astype(np.int64) - state_len
    best = alpha[np.arange(N), last]
    if not traceback:
        return None, best
    align = np.full((N, T), -1, np.int32)
    pos = last.copy()
    ok = last <= T
    rows = np.arange(N)
    for t in range(T - 1, -1, -1):
        align[ok, t] = pos[ok]
        pos = pos - (moved[t, rows, pos] & ok)
    return align, best


def path_score(scores, targets, lengths, state_len, layout_5s, align, blank=None):
    """fp64 score of the alignment `align` [N, T] (position after each step, position 0 before step 0), recomputed from the scores."""
    stay_idx, move_idx = edge_indices(targets, state_len, layout_5s)
    N, T = align.shape
    rows = np.arange(N)
    total = np.zeros(N, np.float64)
    prev = np.zeros(N, np.int64)
    for t in range(T):
        cur = align[:, t].astype(np.int64)
        row = np.asarray(scores[:, t, :])
        is_move = cur == prev + 1
        assert (is_move | (cur == prev)).all()
        stay = row[rows, stay_idx[rows, cur]].astype(np.float64) if stay_idx is not None else np.float64(blank)
        mv = row[rows, move_idx[rows, np.maximum(cur - 1, 0)]].astype(np.float64) if move_idx.shape[1] else 0.0
        total += np.where(is_move, mv, stay)
        prev = cur
    return total


def dense_logz(scores, state_len, layout_5s, blank=None, dtype=np.float64):
    """CTC_CRF.logZ (crf/model.py:47-52) per chunk over all S states, either layout, in `dtype` (fp32 = the reference-order scan)."""
    S = 4 ** state_len
    N, T = scores.shape[0], scores.shape[1]
    j = np.arange(S)
    pred = np.stack([r * (S // 4) + j // 4 for r in range(4)], axis=1)
    alpha = np.zeros((N, S), dtype)
    for t in range(T):
        row = np.asarray(scores[:, t, :]).astype(dtype).reshape(N, S, 5 if layout_5s else 4)
        stay = row[:, :, 0] if layout_5s else dtype(blank)
        mv = row[:, :, 1:] if layout_5s else row
        cand = np.concatenate([(alpha + stay)[:, :, None], alpha[:, pred] + mv], axis=2)
        alpha = np.logaddexp.reduce(cand, axis=2).astype(dtype)
    return np.logaddexp.reduce(alpha, axis=1)


def enumerate_alignments(scores_tc, target_row, length, state_len, layout_5s, blank=None):
    """Brute force over every monotone alignment of ONE chunk [T, C]: (logsumexp of path scores, best score, best align) in fp64.
    Among equal-score paths the one preferred is the kernel's: walking back from the end, stay wherever stay ties."""
    sc = np.asarray(scores_tc, np.float64)[None]
    stay_idx, move_idx = edge_indices(np.asarray(target_row)[None, :length], state_len, layout_5s)
    T, n = sc.shape[1], length + 1 - state_len
    if n - 1 > T:
        return -np.inf, -np.inf, None
    totals, best, best_al = [], -np.inf, None
    for steps in itertools.combinations(range(T), n - 1):          # the steps at which the path moves
        pos, s, al = 0, 0.0, []
        for t in range(T):
            if t in steps:
                s += sc[0, t, move_idx[0, pos]]
                pos += 1
            else:
                s += sc[0, t, stay_idx[0, pos]] if stay_idx is not None else blank
            al.append(pos)
        totals.append(s)
        # the traceback decides the LAST step first and stays on a tie: among equal paths, the largest align read from the end
        if s > best or (s == best and al[::-1] > best_al[::-1]):
            best, best_al = s, al
    return np.logaddexp.reduce(totals), best, np.array(best_al, np.int32)


def free_start_logz(scores_tc, seq, state_len, blank, dtype=np.float64):
    """ln sum over every start state and every alignment emitting exactly `seq` (base indices 0..3) of exp(path score), one chunk of
    koi-layout scores [T, 4S], on the full lattice A[emitted][state], every level in one numpy step. In `dtype`: fp64 is the yardstick;
    run in fp32 it is the fp32 scan of rows that have no fixed-start chain (shorter than k). -inf, never NaN, where len(seq) > T."""
    sc = np.asarray(scores_tc).astype(dtype)
    seq = np.asarray(seq, np.int64).reshape(-1)
    T, S, L = sc.shape[0], 4 ** state_len, len(seq)
    q = S // 4
    states = np.arange(S)
    pred = np.stack([r * q + states // 4 for r in range(4)], axis=1)          # [S, 4]
    enters = states[None, :] % 4 == seq[:, None]                              # [L, S]: level i is entered by emitting seq[i - 1]
    A = np.full((L + 1, S), -np.inf, dtype)
    A[0] = 0
    with np.errstate(invalid="ignore"):
        for t in range(T):
            row = sc[t].reshape(S, 4)
            new = (A + dtype(blank)).astype(dtype)
            if L:
                inc = np.logaddexp.reduce(A[:-1][:, pred] + row[None], axis=2)
                new[1:] = np.logaddexp(new[1:], np.where(enters, inc, dtype(-np.inf)))
            A = new.astype(dtype)
        return np.logaddexp.reduce(A[L])


# ---- torch restatement of koi.ctc.logZ_cu / viterbi_alignments (the reference-order scan) ----------------------------------------

def _torch_log_step(alpha, stay, move):
    import torch
    inc = torch.cat([alpha.new_full((alpha.shape[0], 1), -float("inf")), alpha[:, :-1] + move], dim=1)
    return torch.logaddexp(alpha + stay, inc)


def torch_logz_cu(stay_scores, move_scores, target_lengths):
    """koi.ctc.logZ_cu [EXT]: stay_scores [T, N, n], move_scores [T, N, n-1], target_lengths = chain lengths n_i -> alpha_T[n_i - 1],
    in the dtype of the scores (the reference hands it fp32)."""
    import torch
    T, N, n = stay_scores.shape
    alpha = stay_scores.new_full((N, n), -float("inf"))
    alpha[:, 0] = 0.0
    for t in range(T):
        alpha = _torch_log_step(alpha, stay_scores[t], move_scores[t])
    return alpha.gather(1, (target_lengths.long() - 1)[:, None])[:, 0]


def torch_log_scan_gather(scores_tnc, targets, lengths, state_len, layout_5s, blank=None, dtype=None):
    """The same recurrence, gathering the edges per step from scores [T, N, C] (a torch tensor or view)."""
    import torch
    dtype = dtype or torch.float32
    stay_idx, move_idx = edge_indices(np.asarray(targets), state_len, layout_5s)
    move_idx = torch.from_numpy(move_idx)
    stay_idx = torch.from_numpy(stay_idx) if stay_idx is not None else None
    T, N = scores_tnc.shape[:2]
    alpha = torch.full((N, move_idx.shape[1] + 1), -float("inf"), dtype=dtype)
    alpha[:, 0] = 0.0
    for t in range(T):
        row = scores_tnc[t].to(dtype)
        stay = row.gather(1, stay_idx) if stay_idx is not None else torch.tensor(blank, dtype=dtype)
        alpha = _torch_log_step(alpha, stay, row.gather(1, move_idx))
    last = torch.as_tensor(np.asarray(lengths)).long() - state_len
    return alpha.gather(1, last[:, None])[:, 0]


def torch_viterbi_alignments(stay_scores, move_scores, target_lengths):
    """koi.ctc.viterbi_alignments [EXT] in this project's compact form: int32 [N, T], ties stay."""
    import torch
    T, N, n = stay_scores.shape
    alpha = stay_scores.new_full((N, n), -float("inf"))
    alpha[:, 0] = 0.0
    moved = torch.zeros((T, N, n), dtype=torch.bool)
    for t in range(T):
        inc = torch.cat([alpha.new_full((N, 1), -float("inf")), alpha[:, :-1] + move_scores[t]], dim=1)
        st = alpha + stay_scores[t]
        moved[t] = inc > st
        alpha = torch.where(moved[t], inc, st)
    pos = target_lengths.long() - 1
    ok = pos <= T
    align = torch.full((N, T), -1, dtype=torch.int32)
    rows = torch.arange(N)
    for t in range(T - 1, -1, -1):
        align[ok, t] = pos[ok].to(torch.int32)
        pos = pos - (moved[t, rows, pos] & ok).long()
    return align

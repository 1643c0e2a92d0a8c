"""Test-side alpha-beta restatements of the two gradients of bonito_amd/csrc/seqdist_grad.hip, TEST INFRASTRUCTURE ONLY.

numpy, parameterised by ``dtype``: fp64 is the truth; fp32, in the reference's order (the recurrence of seqdist_ref.log_scan /
dense_logz, whose fp32 run is the reference-order scan, and its mirror), is the yardstick the GPU tolerance is measured from. No
autograd anywhere: the torch restatement's backward is NaN at unreachable positions (logaddexp(-inf, -inf)).

* ``chain_grad``: posterior edge occupancy of the target chain, scattered onto the score elements the edges gather.
* ``chain_grad_banded``: the same numbers bit for bit (logz, grad, share), computed row by row over the reachable cells only.
* ``dense_grad``: posteriors of CTC_CRF.logZ (every edge of every state).
* ``torch_dense_posteriors``: the reference's own expression for SequenceDist.posteriors - autograd of its logZ scan, as the koi
  stub of tests/golden/make_golden.py computes it (dense: every state is reachable, so autograd is safe there).

Layouts: ``scores`` is indexed [n, t, c] here, as in seqdist_ref; the gradients come back the same way."""
import numpy as np

import seqdist_ref as sr


def chain_grad(scores, targets, lengths, state_len, layout_5s, blank=None, dtype=np.float64, weight=None):
    """-> dict(logz [N], grad [N, T, C], stay_total [N, T], move_total [N, T], share [N] int).
    grad[n, t, c] = weight[n] * sum of the posteriors of the edges of step t whose score element is c; a chunk whose target cannot
    fit (logz = -inf) has a zero gradient. stay_total + move_total = the posterior mass of a step (1 for a reachable chunk).
    share[n] = the largest number of chain edges of chunk n that gather one element."""
    stay_idx, move_idx = sr.edge_indices(targets, state_len, layout_5s)
    N, T, C = scores.shape
    n = move_idx.shape[1] + 1
    npos = np.asarray(lengths).astype(np.int64) + 1 - state_len
    rows = np.arange(N)
    alphas = np.empty((T + 1, N, n), dtype)
    alpha = np.full((N, n), -np.inf, dtype)
    alpha[:, 0] = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T):
            alphas[t] = alpha
            stay, move = sr._edges_at(scores, t, stay_idx, move_idx, blank, dtype)
            inc = np.concatenate([np.full((N, 1), -np.inf, dtype), alpha[:, :-1] + move], axis=1)
            alpha = np.logaddexp(alpha + stay, inc).astype(dtype)
        logz = alpha[rows, npos - 1]
        ok = np.isfinite(logz)
        beta = np.full((N, n), -np.inf, dtype)
        beta[rows, npos - 1] = 0
        grad = np.zeros((N, T, C), dtype)
        stay_total = np.zeros((N, T), dtype)
        move_total = np.zeros((N, T), dtype)
        w = np.ones(N, dtype) if weight is None else np.asarray(weight).astype(dtype)
        lz = np.where(ok, logz, 0).astype(dtype)[:, None]
        for t in range(T - 1, -1, -1):
            stay, move = sr._edges_at(scores, t, stay_idx, move_idx, blank, dtype)
            st = (stay + beta).astype(dtype)                                   # stay_t[j] + beta_{t+1}[j]
            inn = (move + beta[:, 1:]).astype(dtype)                           # move_t[j + 1] + beta_{t+1}[j + 1], the edge j -> j + 1
            ps = np.where(ok[:, None], np.exp(alphas[t] + st - lz), 0).astype(dtype)
            pm = np.where(ok[:, None], np.exp(alphas[t][:, :-1] + inn - lz), 0).astype(dtype)
            ps, pm = np.nan_to_num(ps, nan=0.0), np.nan_to_num(pm, nan=0.0)
            stay_total[:, t], move_total[:, t] = ps.sum(axis=1), pm.sum(axis=1)
            if stay_idx is not None:
                np.add.at(grad[:, t, :], (rows[:, None], stay_idx), ps * w[:, None])
            if n > 1:
                np.add.at(grad[:, t, :], (rows[:, None], move_idx), pm * w[:, None])
            beta = np.logaddexp(st, np.concatenate([inn, np.full((N, 1), -np.inf, dtype)], axis=1)).astype(dtype)
    share = np.zeros(N, np.int64)
    for i in range(N):
        used = [] if stay_idx is None else [stay_idx[i, :npos[i]]]
        used.append(move_idx[i, :max(npos[i] - 1, 0)])
        used = np.concatenate(used)
        share[i] = np.bincount(used).max() if used.size else 0
    return {"logz": logz, "grad": grad, "stay_total": stay_total, "move_total": move_total, "share": share}


def chain_grad_banded(scores, targets, lengths, state_len, layout_5s, blank=None, dtype=np.float64, weight=None):
    """chain_grad, row by row and only over the cells a path can pass: before step t a row of `npos` positions is alive at
    max(0, npos - 1 - (T - t)) <= j <= min(npos - 1, t) - to the left of that band the end is out of reach (beta = -inf), to the
    right nothing has arrived (alpha = -inf), and either way chain_grad adds an exact zero there. Inside the band every operation is
    chain_grad's own, on the same operands, in the same order, so the result is bit for bit chain_grad's in either dtype
    (tests/test_seqdist_grad_cpu.py asserts that) at a cost of rows x T x band instead of rows x T x Lmax: what makes a 4096-position
    case with T = Lmax + 3 a matter of a second."""
    stay_idx, move_idx = sr.edge_indices(targets, state_len, layout_5s)
    N, T, C = scores.shape
    lens = np.asarray(lengths).astype(np.int64)
    w = np.ones(N, dtype) if weight is None else np.asarray(weight).astype(dtype)
    logz = np.full(N, -np.inf, dtype)
    grad = np.zeros((N, T, C), dtype)
    stay_total = np.zeros((N, T), dtype)
    move_total = np.zeros((N, T), dtype)
    share = np.zeros(N, np.int64)
    ninf = np.full(1, -np.inf, dtype)
    for i in range(N):
        npos = int(lens[i]) + 1 - state_len
        si = None if stay_idx is None else stay_idx[i, :npos]
        mi = move_idx[i, :npos - 1]
        used = np.concatenate(([] if si is None else [si]) + [mi])
        share[i] = np.bincount(used).max() if used.size else 0
        if npos - 1 > T:
            continue
        x = np.asarray(scores[i])
        lo = [max(0, npos - 1 - (T - t)) for t in range(T + 1)]
        hi = [min(npos - 1, t) for t in range(T + 1)]

        def stays(t, a, b):                                                    # the stay edges of positions a .. b
            return x[t, si[a:b + 1]].astype(dtype) if si is not None else dtype(blank)

        alpha = np.full(npos, -np.inf, dtype)
        alpha[0] = 0
        kept = []
        for t in range(T):
            kept.append(alpha[lo[t]:hi[t] + 1].copy())
            a, b = lo[t + 1], hi[t + 1]                                        # the band after the step
            stay = stays(t, a, b)
            first = max(a, 1)                                                  # mi[j - 1] scores the edge into position j >= 1
            inc = (alpha[first - 1:b] + x[t, mi[first - 1:b]].astype(dtype)).astype(dtype)
            if a == 0:
                inc = np.concatenate([ninf, inc])
            alpha[a:b + 1] = np.logaddexp(alpha[a:b + 1] + stay, inc).astype(dtype)
        logz[i] = alpha[npos - 1]
        lz = logz[i]
        beta = np.full(npos + 1, -np.inf, dtype)                               # (one past the end: no edge leaves the last position)
        beta[npos - 1] = 0
        for t in range(T - 1, -1, -1):
            a, b = lo[t], hi[t]
            stay = stays(t, a, b)
            move = x[t, mi[a:b + 1]].astype(dtype)                             # the edges j -> j + 1 for a <= j <= min(b, npos - 2)
            m = move.shape[0]
            st = (stay + beta[a:b + 1]).astype(dtype)
            inn = (move + beta[a + 1:a + 1 + m]).astype(dtype)
            ps = np.exp(kept[t] + st - lz).astype(dtype)
            pm = np.exp(kept[t][:m] + inn - lz).astype(dtype)
            stay_total[i, t], move_total[i, t] = ps.sum(), pm.sum()
            if si is not None:
                np.add.at(grad[i, t], si[a:b + 1], ps * w[i])
            np.add.at(grad[i, t], mi[a:a + m], pm * w[i])
            beta[a:b + 1] = np.logaddexp(st, np.concatenate([inn, ninf]) if m == b - a else inn).astype(dtype)
    return {"logz": logz, "grad": grad, "stay_total": stay_total, "move_total": move_total, "share": share}


def dense_grad(scores, state_len, layout_5s, blank=None, dtype=np.float64, weight=None):
    """-> (logZ [N], grad [N, T, C]): grad[n, t, 5 s' + 0] = w exp(alpha_t[s'] + stay + beta_{t+1}[s'] - logZ) and
    grad[n, t, 5 s' + 1 + r] = w exp(alpha_t[r S/4 + s'/4] + move_t[s'][r] + beta_{t+1}[s'] - logZ) (koi layout: 4 s' + r only)."""
    S = 4 ** state_len
    q = S // 4
    N, T, C = scores.shape
    W = 5 if layout_5s else 4
    j = np.arange(S)
    pred = np.stack([r * q + j // 4 for r in range(4)], axis=1)               # [S, 4]
    succ = np.stack([(j % q) * 4 + b for b in range(4)], axis=1)             # [S, 4]: successors of j, each through r = j // q
    alphas = np.empty((T + 1, N, S), dtype)
    alpha = np.zeros((N, S), dtype)
    rowsT = []
    for t in range(T):
        alphas[t] = alpha
        row = np.asarray(scores[:, t, :]).astype(dtype).reshape(N, S, W)
        rowsT.append(row)
        stay = row[:, :, 0] if layout_5s else dtype(blank)
        mv = row[:, :, 1:] if layout_5s else row
        cand = np.concatenate([(alpha + stay)[:, :, None], alpha[:, pred] + mv], axis=2)
        alpha = np.logaddexp.reduce(cand, axis=2).astype(dtype)
    logz = np.logaddexp.reduce(alpha, axis=1).astype(dtype)
    w = np.ones(N, dtype) if weight is None else np.asarray(weight).astype(dtype)
    beta = np.zeros((N, S), dtype)
    grad = np.empty((N, T, S, W), dtype)
    for t in range(T - 1, -1, -1):
        row = rowsT[t]
        stay = row[:, :, 0] if layout_5s else dtype(blank)
        mv = row[:, :, 1:] if layout_5s else row
        e = (mv + beta[:, :, None]).astype(dtype)                              # [N, S', 4]
        base = (beta - logz[:, None]).astype(dtype)
        if layout_5s:
            grad[:, t, :, 0] = w[:, None] * np.exp(alphas[t] + stay + base)
        grad[:, t, :, W - 4:] = w[:, None, None] * np.exp(alphas[t][:, pred] + mv + base[:, :, None])
        cand = np.concatenate([(stay + beta)[:, :, None], e[:, succ, (j // q)[:, None]]], axis=2)
        beta = np.logaddexp.reduce(cand, axis=2).astype(dtype)
    return logz, grad.reshape(N, T, C)


def torch_dense_posteriors(scores_tnc, state_len):
    """The reference's SequenceDist.posteriors (Log semiring) for [T, N, 5S] scores: autograd of CTC_CRF.logZ's scan
    alpha_{t+1}[n, j] = logsumexp_k(Ms[t, n, j, k] + alpha_t[n, idx[j, k]]), in fp64 on the CPU."""
    import torch
    S = 4 ** state_len
    states = torch.arange(S)
    idx = torch.cat([states[:, None], states.repeat_interleave(4).reshape(4, -1).T], dim=1)
    x = torch.as_tensor(np.asarray(scores_tnc)).double().clone().requires_grad_(True)
    T, N, _ = x.shape
    Ms = x.reshape(T, N, -1, 5)
    alpha = Ms.new_zeros((N, S))
    for t in range(T):
        alpha = torch.logsumexp(Ms[t] + alpha[:, idx], dim=-1)
    (g,) = torch.autograd.grad(torch.logsumexp(alpha, dim=-1).sum(), x)
    return g.numpy()

"""Restatement of the CTC loss of bonito.ctc (torch.nn.functional.ctc_loss behind Model.ctc_label_smoothing_loss, reference
bonito/ctc/model.py:48-57) as an alpha-beta pass in numpy, fp64 by default: what csrc/ctc_loss.hip is tested against.

Definition (torch's, blank = class 0): l' = the target with blanks interleaved, S = 2 len + 1 states,
    alpha_0[0] = lp_0[0], alpha_0[1] = lp_0[l'_1],
    alpha_t[s] = lp_t[l'_s] + logsumexp(alpha_{t-1}[s], alpha_{t-1}[s-1], alpha_{t-1}[s-2])    (s-2 only when l'_s != 0, l'_s != l'_{s-2})
    nll = -logaddexp(alpha_{T-1}[S-1], alpha_{T-1}[S-2]);   beta = the mirror scan;
    occ[t][c] = sum over the states s with l'_s = c of P(the path is in s at step t | target) = -d nll / d lp[t][c].
This project's definitions where torch yields NaN:
  * no alignment (len + adjacent repeats > T, or every alignment crosses a -inf log-prob): nll = +inf, occ = 0;
  * a state that a -inf log-prob makes unreachable contributes occupancy 0;
  * len outside 0..Lmax or a label outside 1..C-1: nll = NaN, occ = 0 (the kernel writes no gradient there).
smooth[n] = sum_t sum_c w_c lp[t][n][c] over the classes with w_c != 0."""
import numpy as np


def _lse(*xs):
    out = xs[0]
    for x in xs[1:]:
        out = np.logaddexp(out, x)
    return out


def _shift(x, k, fill):
    """x moved by k places towards higher (k > 0) or lower (k < 0) indices, `fill` where nothing arrives"""
    out = np.full_like(x, fill)
    n = len(x)
    if k > 0 and n > k:
        out[k:] = x[:n - k]
    if k < 0 and n > -k:
        out[:n + k] = x[-k:]
    return out


def ctc_chunk(lp, target, dtype=np.float64):
    """lp [T, C], target [len] -> (nll, occ [T, C], occ_states [T, S]) in `dtype`."""
    lp = np.asarray(lp, dtype)
    T, C = lp.shape
    target = np.asarray(target, np.int64)
    S = 2 * len(target) + 1
    ext = np.zeros(S, np.int64)
    ext[1::2] = target
    ninf = dtype(-np.inf)
    skip = np.zeros(S, bool)
    if S > 3:
        skip[3::2] = ext[3::2] != ext[1:-2:2]
    em = lp[:, ext]                                                         # [T, S]
    with np.errstate(invalid="ignore", over="ignore"):
        alpha = np.full((T, S), ninf, dtype)
        prev = np.full(S, ninf, dtype)
        prev[0] = 0                                                         # "alpha_{-1}"
        for t in range(T):
            a1 = _shift(prev, 1, ninf)
            a2 = np.where(skip, _shift(prev, 2, ninf), ninf)
            prev = (em[t] + _lse(prev, a1, a2)).astype(dtype)
            prev[np.isnan(prev)] = ninf                                     # (-inf) + (-inf) paths of numpy's logaddexp are fine; guard inf - inf
            alpha[t] = prev
        logz = _lse(alpha[-1, S - 1], alpha[-1, S - 2]) if S > 1 else alpha[-1, 0]
        occ_s = np.zeros((T, S), dtype)
        occ = np.zeros((T, C), dtype)
        if not np.isfinite(logz):
            return dtype(np.inf), occ, occ_s
        skipf = np.zeros(S, bool)
        if S > 2:
            skipf[:-2] = skip[2:]                                               # from s to s + 2
        nxt = np.full(S, ninf, dtype)
        nxt[S - 1] = 0                                                      # "beta_T"
        for t in range(T - 1, -1, -1):
            b1 = _shift(nxt, -1, ninf)
            b2 = np.where(skipf, _shift(nxt, -2, ninf), ninf)
            bp = _lse(nxt, b1, b2).astype(dtype)                            # the log-sum over the successors, without lp_t
            occ_s[t] = np.exp(alpha[t] + bp - logz)
            nxt = (em[t] + bp).astype(dtype)
            nxt[np.isnan(nxt)] = ninf
        occ_s[np.isnan(occ_s)] = 0
        np.add.at(occ, (np.arange(T)[:, None], ext[None, :]), occ_s)
    return dtype(-logz), occ, occ_s


def ctc_loss_ref(log_probs, targets, lengths, weights=None, dtype=np.float64):
    """log_probs [T, N, C], targets [N, Lmax], lengths [N] -> dict(nll [N], occ [T, N, C], smooth [N] or None)."""
    log_probs = np.asarray(log_probs, dtype)
    T, N, C = log_probs.shape
    targets = np.asarray(targets).reshape(N, -1)
    nll = np.zeros(N, dtype)
    occ = np.zeros((T, N, C), dtype)
    for n in range(N):
        ln = int(lengths[n])
        tg = targets[n, :max(ln, 0)].astype(np.int64)
        if ln < 0 or ln > targets.shape[1] or (tg < 1).any() or (tg >= C).any():
            nll[n] = np.nan
            continue
        nll[n], occ[:, n], _ = ctc_chunk(log_probs[:, n], tg, dtype)
    smooth = None
    if weights is not None:
        w = np.asarray(weights, dtype)
        use = w != 0
        smooth = (log_probs[:, :, use] * w[use]).sum(axis=(0, 2))
    return {"nll": nll, "occ": occ, "smooth": smooth}


def default_weights(C):
    """[0.4, 0.1 / (C - 1), ...] as the reference builds them: fp32 tensors (ctc/model.py:50)"""
    return np.concatenate([[np.float32(0.4)], np.full(C - 1, np.float32(0.1 / (C - 1)))]).astype(np.float32).astype(np.float64)


def loss_dict(log_probs, targets, lengths, weights=None, reduction="mean", dtype=np.float64):
    """The reference's dict from the restatement: loss = mean_n nll_n / max(len_n, 1), label_smooth_loss = -sum(lp w) / (T N C)."""
    T, N, C = np.asarray(log_probs).shape
    if weights is None:
        weights = default_weights(C)
    r = ctc_loss_ref(log_probs, targets, lengths, weights, dtype)
    per = r["nll"] / np.maximum(np.asarray(lengths), 1)
    loss = per.mean() if reduction == "mean" else per
    ls = -r["smooth"].sum() / (T * N * C)
    return {"total_loss": loss + ls, "loss": loss, "label_smooth_loss": ls}


def logsoftmax_projection(g, lp):
    """log_softmax's backward: the gradient with respect to the logits from the gradient g with respect to lp = log_softmax(logits)."""
    return g - np.exp(lp) * g.sum(axis=-1, keepdims=True)

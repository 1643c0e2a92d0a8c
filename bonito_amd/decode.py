"""
CRF decoding entry points with the call surface of ``koi.decode`` (the un-vendored dependency the
reference calls at /root/reference bonito/crf/basecall.py:7,36-40,48-55), backed by the HIP kernels in
bonito_amd/csrc/crf.hip through the C ABI (``bh_crf_viterbi`` ...).
"""
import ctypes as C

import numpy as np
import torch

from bonito_amd import _lib

_ALPHABET = np.frombuffer(b"NACGT", dtype=np.uint8)


def _check_scores(scores):
    if scores.dtype != torch.float16:
        raise TypeError("Expected fp16 but received %s" % scores.dtype)   # koi raises TypeError too
    if not scores.is_cuda:
        raise _lib.HipEngineError("scores must live on a HIP device (no CPU decode fallback)")
    if not scores.is_contiguous():
        raise AssertionError("scores must be contiguous [N, T, C]")


def state_len_of(C_, n_base=4):
    """state_len such that C == n_base^(state_len+1) (koi layout, expand_blanks=False)."""
    sl, size = 0, n_base
    while size < C_:
        size *= n_base
        sl += 1
    if size != C_:
        raise ValueError("score width %d is not a power of %d" % (C_, n_base))
    return sl


class CRFDecoder:
    """Pre-allocated decode context (workspace, device + pinned host output planes) for batches of up
    to (max_batch, T, C). ``submit(scores)`` enqueues the HIP decode and the int8 D2H copy on the current
    stream and returns a ticket; ``ticket.result()`` waits and returns CPU tensors. Used by the pipelined
    basecaller / bench so that decode of batch i overlaps the encoder of batch i+1 on another stream."""

    def __init__(self, max_batch, T, C, device, mode="beam", beam_width=32, beam_cut=100.0, scale=1.0, offset=0.0,
                 blank_score=2.0):
        lib = _lib.lib()
        self.mode, self.device = mode, torch.device(device)
        self.N, self.T, self.C = int(max_batch), int(T), int(C)
        self.sl = state_len_of(self.C)
        self.args = (int(beam_width), float(beam_cut), float(blank_score), float(scale), float(offset))
        nbytes = (lib.bh_beam_search_workspace(self.N, self.T, self.sl) if mode == "beam"
                  else lib.bh_crf_viterbi_workspace(self.N, self.T, self.sl))
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.dev_out = torch.empty((3, self.N, self.T), dtype=torch.int8, device=self.device)
        self.host_out = torch.empty((3, self.N, self.T), dtype=torch.int8).pin_memory()
        self.done = torch.cuda.Event()

    class Ticket:
        def __init__(self, dec, n):
            self.dec, self.n = dec, n

        def result_planes(self):
            """CPU int8 [3, N, T] = (sequence, qstring, moves) stacked (a copy, safe to keep)."""
            self.dec.done.synchronize()
            h = self.dec.host_out[:, : self.n]
            # plain pageable copy, single-threaded on purpose: .clone() of a pinned tensor would hipHostMalloc a new
            # pinned block (~6 ms), and torch's parallel CPU copy wakes the whole intra-op pool for 2.5 MB
            return torch.from_numpy(np.array(h.numpy(), copy=True))

        def result(self):
            """(sequence, qstring, moves) CPU int8 [N, T] (copies, safe to keep)."""
            out = self.result_planes()
            return out[0], out[1], out[2]

    def submit(self, scores):
        _check_scores(scores)
        N, T, Cc = scores.shape
        if N > self.N or T != self.T or Cc != self.C:
            raise ValueError("decoder built for (<=%d, %d, %d), got %s" % (self.N, self.T, self.C, tuple(scores.shape)))
        lib = _lib.lib()
        bw, cut, blank, scale, offset = self.args
        out = self.dev_out
        with torch.cuda.device(self.device):
            st = _lib.stream_ptr(self.device)
            if self.mode == "beam":
                _lib.check(lib.bh_beam_search(_lib.ptr(scores), N, T, self.sl, bw, cut, blank, scale, offset,
                                              _lib.ptr(self.ws), _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]),
                                              None, st), "bh_beam_search")
                for pl in range(3):      # one dense copy per plane: a [3, :N] slice is strided when N < max_batch
                    self.host_out[pl, :N].copy_(out[pl, :N], non_blocking=True)
            else:
                # viterbi: plane 2 = moves, plane 1 = path (0..4); sequence/qstring are derived on the host
                _lib.check(lib.bh_crf_viterbi(_lib.ptr(scores), N, T, self.sl, 0, blank, T * Cc, Cc, _lib.ptr(self.ws),
                                              _lib.ptr(out[2]), _lib.ptr(out[1]), None, st), "bh_crf_viterbi")
                for pl in (1, 2):
                    self.host_out[pl, :N].copy_(out[pl, :N], non_blocking=True)
            self.done.record(torch.cuda.current_stream(self.device))
        return CRFDecoder.Ticket(self, N)


def beam_search(scores, beam_width=32, beam_cut=100.0, scale=1.0, offset=0.0, blank_score=2.0, return_qfloat=False):
    """koi.decode.beam_search replacement (same arguments and defaults, bonito/crf/basecall.py:27,36-40).
    scores: cuda fp16 contiguous [N, T, 4^(state_len+1)].  Returns CPU int8 tensors
    (sequence, qstring, moves), each [N, T] with zeros where no base is emitted."""
    _check_scores(scores)
    N, T, Cc = scores.shape
    sl = state_len_of(Cc)
    lib = _lib.lib()
    dev = scores.device
    ws = torch.empty(lib.bh_beam_search_workspace(N, T, sl), dtype=torch.uint8, device=dev)
    out = torch.empty((3, N, T), dtype=torch.int8, device=dev)
    qf = torch.empty((N, T), dtype=torch.float32, device=dev) if return_qfloat else None
    with torch.cuda.device(dev):
        _lib.check(lib.bh_beam_search(_lib.ptr(scores), N, T, sl, int(beam_width), float(beam_cut), float(blank_score),
                                      float(scale), float(offset), _lib.ptr(ws), _lib.ptr(out[0]), _lib.ptr(out[1]),
                                      _lib.ptr(out[2]), _lib.ptr(qf), _lib.stream_ptr(dev)), "bh_beam_search")
    host = out.cpu()          # one D2H copy of the three int8 planes (koi also returns CPU tensors)
    if return_qfloat:
        return host[0], host[1], host[2], qf.cpu()
    return host[0], host[1], host[2]


def viterbi(scores, blank_score=2.0, return_score=False):
    """Max-semiring best path of the CTC-CRF (CTC_CRF.viterbi, bonito/crf/model.py:98-103) on koi-layout
    scores fp16 [N, T, 4^(state_len+1)].  Returns CPU int8 tensors (moves [N,T] in {0,1},
    path [N,T] in {0..4}), like koi's decoders return CPU int8."""
    _check_scores(scores)
    N, T, Cc = scores.shape
    sl = state_len_of(Cc)
    lib = _lib.lib()
    dev = scores.device
    ws = torch.empty(lib.bh_crf_viterbi_workspace(N, T, sl), dtype=torch.uint8, device=dev)
    moves = torch.empty((N, T), dtype=torch.int8, device=dev)
    path = torch.empty((N, T), dtype=torch.int8, device=dev)
    best = torch.empty((N,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.bh_crf_viterbi(_lib.ptr(scores), N, T, sl, 0, float(blank_score), T * Cc, Cc, _lib.ptr(ws),
                                      _lib.ptr(moves), _lib.ptr(path), _lib.ptr(best), _lib.stream_ptr(dev)),
                   "bh_crf_viterbi")
    if return_score:
        return moves.cpu(), path.cpu(), best.cpu()
    return moves.cpu(), path.cpu()


def viterbi_5s(scores_tnc, state_len, return_score=False):
    """Same, on the reference's expand_blanks layout: fp16 [T, N, 5*4^state_len] (crf/model.py:49)."""
    if scores_tnc.dtype != torch.float16 or not scores_tnc.is_cuda:
        raise TypeError("expected cuda fp16 scores")
    scores_tnc = scores_tnc.contiguous()
    T, N, Cc = scores_tnc.shape
    lib = _lib.lib()
    dev = scores_tnc.device
    ws = torch.empty(lib.bh_crf_viterbi_workspace(N, T, state_len), dtype=torch.uint8, device=dev)
    moves = torch.empty((N, T), dtype=torch.int8, device=dev)
    path = torch.empty((N, T), dtype=torch.int8, device=dev)
    best = torch.empty((N,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.bh_crf_viterbi(_lib.ptr(scores_tnc), N, T, state_len, 1, 0.0, Cc, N * Cc, _lib.ptr(ws),
                                      _lib.ptr(moves), _lib.ptr(path), _lib.ptr(best), _lib.stream_ptr(dev)),
                   "bh_crf_viterbi")
    if return_score:
        return moves.cpu(), path.cpu(), best.cpu()
    return moves.cpu(), path.cpu()


def path_to_sequence(path):
    """int8 path in {0..4} -> int8 ASCII bytes (0 where nothing is emitted): koi's `sequence` layout,
    so ``to_str`` and ``stitch`` (crf/basecall.py:13-24,48-55) work on it unchanged."""
    p = path.numpy() if isinstance(path, torch.Tensor) else np.asarray(path)
    out = np.where(p != 0, _ALPHABET[p.astype(np.int64)], 0).astype(np.int8)
    return torch.from_numpy(out)


def to_str(x, encoding="ascii"):
    """Non-zero bytes decoded as text (koi.decode.to_str)."""
    a = x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    a = a[a != 0]
    return a.astype(np.uint8).tobytes().decode(encoding)


def reverse_complement(scores):
    """CTC_CRF.reverse_complement (bonito/crf/model.py:84-96) on koi-layout scores cuda fp16 [N, T, 4S]."""
    _check_scores(scores)
    N, T, Cc = scores.shape
    out = torch.empty_like(scores)
    with torch.cuda.device(scores.device):
        _lib.check(_lib.lib().bh_crf_reverse_complement(_lib.ptr(scores), _lib.ptr(out), N, T, state_len_of(Cc), 0,
                                                        T * Cc, Cc, _lib.stream_ptr(scores.device)), "bh_crf_reverse_complement")
    return out


def reverse_complement_5s(scores_tnc, state_len):
    """Same on the reference layout [T, N, 5S] (cuda fp16)."""
    scores_tnc = scores_tnc.contiguous()
    T, N, Cc = scores_tnc.shape
    out = torch.empty_like(scores_tnc)
    with torch.cuda.device(scores_tnc.device):
        _lib.check(_lib.lib().bh_crf_reverse_complement(_lib.ptr(scores_tnc), _lib.ptr(out), N, T, int(state_len), 1,
                                                        Cc, N * Cc, _lib.stream_ptr(scores_tnc.device)), "bh_crf_reverse_complement")
    return out


def logz(scores, blank_score=2.0):
    """Log-partition function per chunk (CTC_CRF.logZ, crf/model.py:47-52) of koi-layout scores -> CPU float64 [N]."""
    _check_scores(scores)
    N, T, Cc = scores.shape
    sl = state_len_of(Cc)
    lib = _lib.lib()
    ws = torch.empty(lib.bh_beam_search_workspace(N, T, sl), dtype=torch.uint8, device=scores.device)
    out = torch.empty(N, dtype=torch.float64, device=scores.device)
    with torch.cuda.device(scores.device):
        _lib.check(lib.bh_crf_logz(_lib.ptr(scores), N, T, sl, float(blank_score), _lib.ptr(ws), _lib.ptr(out),
                                   _lib.stream_ptr(scores.device)), "bh_crf_logz")
    return out.cpu()


def posterior_viterbi(scores, blank_score=2.0):
    """SeqdistModel.decode_batch's decoder (crf/model.py:196-199): best path over log edge posteriors.
    scores cuda fp16 [N, T, 4S] -> CPU int8 (moves, path)."""
    _check_scores(scores)
    N, T, Cc = scores.shape
    sl = state_len_of(Cc)
    lib = _lib.lib()
    dev = scores.device
    ws = torch.empty(lib.bh_crf_posterior_viterbi_workspace(N, T, sl), dtype=torch.uint8, device=dev)
    moves = torch.empty((N, T), dtype=torch.int8, device=dev)
    path = torch.empty((N, T), dtype=torch.int8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.bh_crf_posterior_viterbi(_lib.ptr(scores), N, T, sl, float(blank_score), _lib.ptr(ws),
                                                _lib.ptr(moves), _lib.ptr(path), _lib.stream_ptr(dev)), "bh_crf_posterior_viterbi")
    return moves.cpu(), path.cpu()


def set_option(name, value):
    """Process-wide engine knob (bh_set_option), e.g. set_option("beam_fork", 0)."""
    _lib.check(_lib.lib().bh_set_option(name.encode(), int(value)), "bh_set_option")


# ---- sequence likelihood and forced alignment (csrc/seqdist.hip) -------------------------------------------------------------

def seq_layout(scores, state_len, blank_score=None):
    """(N, T, layout_5s, stride_n, stride_t) of a score tensor for the bh_crf_seq_* entry points: the reference layout
    [T, N, 5S] (expand_blanks, crf/model.py:49) or the engine's koi layout [N, T, 4S], which needs `blank_score`.
    Strided / offset views are passed as they are (element strides); only the score axis must be dense."""
    S = 4 ** int(state_len)
    if scores.dim() != 3 or scores.shape[-1] not in (4 * S, 5 * S):
        raise ValueError("scores of shape %s are neither [T, N, %d] nor [N, T, %d] (state_len %d)"
                         % (tuple(scores.shape), 5 * S, 4 * S, state_len))
    if scores.shape[-1] == 5 * S:
        T, N = scores.shape[:2]
        return N, T, 1, scores.stride(1), scores.stride(0)
    if blank_score is None:
        raise ValueError("koi-layout scores [N, T, %d] need blank_score" % (4 * S))
    N, T = scores.shape[:2]
    return N, T, 0, scores.stride(0), scores.stride(1)


def check_targets(targets, target_lengths, state_len, free_start=False):
    """Argument checks of the sequence scans, on the host and before anything is launched: labels in 0..4, every length within
    [state_len, Lmax] (a free-start row may be shorter, down to 0). Returns (targets int8/int32 [N, Lmax], lengths int32 [N])."""
    if targets.dim() != 2 or target_lengths.dim() != 1 or targets.shape[0] != target_lengths.shape[0]:
        raise ValueError("targets must be [N, Lmax] and target_lengths [N]")
    if targets.dtype not in (torch.int8, torch.int32):
        if targets.dtype.is_floating_point:
            raise TypeError("targets must be integer labels, got %s" % targets.dtype)
        targets = targets.to(torch.int32)
    lengths = target_lengths.to(torch.int32)
    lo, hi = (int(lengths.min()), int(lengths.max())) if lengths.numel() else (0, 0)
    if not free_start and lo < state_len:
        raise ValueError("target length %d is shorter than state_len %d" % (lo, state_len))
    if lo < 0 or hi > targets.shape[1]:
        raise ValueError("target lengths must lie in 0..%d (got %d..%d)" % (targets.shape[1], lo, hi))
    if targets.numel() and (int(targets.min()) < 0 or int(targets.max()) > 4):
        raise ValueError("target labels must lie in 0..4")
    return targets, lengths


def _seq_call(scores, targets, target_lengths, state_len, blank_score, mode):
    if scores.requires_grad:
        from bonito_amd.nn import NoTorchCompute
        raise NoTorchCompute("this entry point returns a plain tensor: for scores with requires_grad use seq_logz_grad / "
                             "CTC_CRF.ctc_loss, which carry the backward")
    N, T, five, s_n, s_t = seq_layout(scores, state_len, blank_score)
    if mode == "free" and five:
        raise ValueError("the free-start sum is defined on koi-layout scores [N, T, 4S]")
    targets, lengths = check_targets(targets, target_lengths, state_len, free_start=(mode == "free"))
    if targets.shape[0] != N:
        raise ValueError("%d target rows for %d chunks" % (targets.shape[0], N))
    if not scores.is_cuda:
        raise _lib.HipEngineError("scores must live on a HIP device (no CPU fallback)")
    if scores.dtype != torch.float16:
        scores = scores.to(torch.float16)
        N, T, five, s_n, s_t = seq_layout(scores, state_len, blank_score)
    if scores.stride(2) != 1:
        scores = scores.contiguous()
        N, T, five, s_n, s_t = seq_layout(scores, state_len, blank_score)
    lib = _lib.lib()
    dev = scores.device
    Lmax = int(targets.shape[1])
    if Lmax == 0:                                   # (free start, every row empty)
        targets, Lmax = torch.zeros((N, 1), dtype=torch.int8), 1
    targets = targets.to(dev).contiguous()
    lengths = lengths.to(dev).contiguous()
    nbytes = lib.bh_crf_seq_workspace(N, T, Lmax, state_len)
    if nbytes == 0:
        raise ValueError("unsupported shape: Lmax + 1 - state_len = %d positions (limit 4096), state_len %d (1..5)"
                         % (Lmax + 1 - state_len, state_len))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(N, dtype=torch.float32, device=dev)
    blank = float(blank_score if blank_score is not None else 0.0)
    tb = targets.element_size()
    with torch.cuda.device(dev):
        st = _lib.stream_ptr(dev)
        if mode == "log":
            _lib.check(lib.bh_crf_seq_logz(_lib.ptr(scores), N, T, state_len, five, blank, s_n, s_t, _lib.ptr(targets), Lmax, tb,
                                           _lib.ptr(lengths), _lib.ptr(ws), _lib.ptr(out), st), "bh_crf_seq_logz")
            return out
        if mode == "free":
            _lib.check(lib.bh_crf_seq_logz_free(_lib.ptr(scores), N, T, state_len, blank, s_n, s_t, _lib.ptr(targets), Lmax, tb,
                                                _lib.ptr(lengths), _lib.ptr(ws), _lib.ptr(out), st), "bh_crf_seq_logz_free")
            return out
        align = torch.empty((N, T), dtype=torch.int32, device=dev)
        _lib.check(lib.bh_crf_seq_viterbi(_lib.ptr(scores), N, T, state_len, five, blank, s_n, s_t, _lib.ptr(targets), Lmax, tb,
                                          _lib.ptr(lengths), _lib.ptr(ws), _lib.ptr(align), _lib.ptr(out), st), "bh_crf_seq_viterbi")
        return align, out


def seq_logz(scores, targets, target_lengths, state_len, blank_score=None, free_start=False):
    """koi.ctc.logZ_cu of the chain of CTC_CRF.prepare_ctc_scores (crf/model.py:110-130), gathered inside the kernel:
    ln of the sum over every alignment of the target, fp32 -> device float32 [N] (-inf where the target cannot fit into T steps).
    free_start=True (koi layout): the sum also runs over every start state - the numerator of ln P(sequence | scores)."""
    return _seq_call(scores, targets, target_lengths, int(state_len), blank_score, "free" if free_start else "log")


def seq_viterbi(scores, targets, target_lengths, state_len, blank_score=None):
    """Forced alignment (koi.ctc.viterbi_alignments, crf/model.py:143): (align int32 [N, T], best float32 [N]) on the CPU.
    align[n, t] = the chain position (k-mer index of the target) occupied after step t; ties resolve to stay; rows whose
    target cannot fit into T steps are -1 with best = -inf. The compact form is this project's own definition (koi is closed)."""
    align, best = _seq_call(scores, targets, target_lengths, int(state_len), blank_score, "max")
    return align.cpu(), best.cpu()


def logz_any(scores, state_len, blank_score=None):
    """CTC_CRF.logZ per chunk for either layout -> device float64 [N]: bh_crf_logz for contiguous koi-layout scores, the dense
    fp32 scan of csrc/seqdist.hip (bh_crf_logz_dense) for the reference layout [T, N, 5S] and for strided views."""
    N, T, five, s_n, s_t = seq_layout(scores, state_len, blank_score)
    if not scores.is_cuda:
        raise _lib.HipEngineError("scores must live on a HIP device (no CPU fallback)")
    if scores.dtype != torch.float16:
        scores = scores.to(torch.float16)
    if scores.stride(2) != 1:
        scores = scores.contiguous()
    N, T, five, s_n, s_t = seq_layout(scores, state_len, blank_score)
    lib = _lib.lib()
    dev = scores.device
    with torch.cuda.device(dev):
        if not five and scores.is_contiguous():
            ws = torch.empty(lib.bh_beam_search_workspace(N, T, state_len), dtype=torch.uint8, device=dev)
            out = torch.empty(N, dtype=torch.float64, device=dev)
            _lib.check(lib.bh_crf_logz(_lib.ptr(scores), N, T, state_len, float(blank_score), _lib.ptr(ws), _lib.ptr(out),
                                       _lib.stream_ptr(dev)), "bh_crf_logz")
            return out
        out = torch.empty(N, dtype=torch.float32, device=dev)
        _lib.check(lib.bh_crf_logz_dense(_lib.ptr(scores), N, T, state_len, five, float(blank_score or 0.0), s_n, s_t,
                                         _lib.ptr(out), _lib.stream_ptr(dev)), "bh_crf_logz_dense")
        return out.double()


def _grad_scores(scores, state_len, blank_score):
    """Device fp16 scores with a dense score axis for the gradient entry points (fp32 is rounded to fp16, as in the forward scans;
    the gradient is then that of the rounded scores). -> (scores fp16, grad dtype)."""
    seq_layout(scores, state_len, blank_score)
    if not scores.is_cuda:
        raise _lib.HipEngineError("scores must live on a HIP device (no CPU fallback)")
    if scores.dtype not in (torch.float16, torch.float32):
        raise TypeError("scores must be fp16 or fp32, got %s" % scores.dtype)
    gdtype = scores.dtype
    scores = scores.detach()
    if scores.dtype != torch.float16:
        scores = scores.to(torch.float16)
    if scores.stride(2) != 1:
        scores = scores.contiguous()
    return scores, gdtype


def _grad_out(out, scores, gdtype, state_len, blank_score):
    """The gradient tensor: a new one shaped like `scores`, or the caller's `out` (fp16 / fp32, same shape, same device, its own
    strides with a dense score axis). -> (out, g_stride_n, g_stride_t, grad_fp32)."""
    if out is None:
        out = torch.empty(scores.shape, dtype=gdtype, device=scores.device)
    else:
        if tuple(out.shape) != tuple(scores.shape) or out.device != scores.device:
            raise ValueError("out must have the shape %s and the device of the scores" % (tuple(scores.shape),))
        if out.dtype not in (torch.float16, torch.float32):
            raise TypeError("out must be fp16 or fp32, got %s" % out.dtype)
        if out.stride(2) != 1:
            raise ValueError("the score axis of out must be dense")
        if out.requires_grad:
            raise ValueError("out must not require grad")
    _, _, _, g_n, g_t = seq_layout(out, state_len, 0.0 if blank_score is None else blank_score)
    return out, g_n, g_t, int(out.dtype == torch.float32)


def _weight(weight, N, dev):
    if weight is None:
        return None
    weight = weight.detach().to(device=dev, dtype=torch.float32).contiguous()
    if weight.shape != (N,):
        raise ValueError("weight must be [N] = [%d]" % N)
    return weight


def seq_logz_grad(scores, targets, target_lengths, state_len, blank_score=None, weight=None, out=None, accumulate=False):
    """seq_logz AND its gradient from one launch (bh_crf_seq_logz_grad): (logz float32 [N], grad), both on the device.
    grad[n, t, c] = weight[n] * the posterior probability that the alignment takes, at step t, an edge whose score is element c
    (positions that share an element are summed). It has the shape and dtype (fp16 / fp32) of `scores`; fp32 scores are rounded to
    fp16 for the kernel and the gradient is that of the rounded scores. ``out``: write into this tensor instead (fp16 or fp32, own
    strides, dense score axis); ``accumulate=True`` adds into it. A chunk whose target cannot fit into T steps has logz = -inf and a
    ZERO gradient (this project's definition). The result is bit-identical from call to call. Koi-layout scores: the stay edge is
    the scalar blank_score and gets no gradient."""
    state_len = int(state_len)
    N, T, five, s_n, s_t = seq_layout(scores, state_len, blank_score)
    targets, lengths = check_targets(targets, target_lengths, state_len)
    if targets.shape[0] != N:
        raise ValueError("%d target rows for %d chunks" % (targets.shape[0], N))
    if accumulate and out is None:
        raise ValueError("accumulate=True needs out")
    scores, gdtype = _grad_scores(scores, state_len, blank_score)
    N, T, five, s_n, s_t = seq_layout(scores, state_len, blank_score)
    out, g_n, g_t, g32 = _grad_out(out, scores, gdtype, state_len, blank_score)
    lib = _lib.lib()
    dev = scores.device
    Lmax = int(targets.shape[1])
    targets = targets.to(dev).contiguous()
    lengths = lengths.to(dev).contiguous()
    weight = _weight(weight, N, dev)
    nbytes = lib.bh_crf_seq_grad_workspace(N, T, Lmax, state_len)
    if nbytes == 0:
        raise ValueError("unsupported shape: Lmax + 1 - state_len = %d positions (limit 4096), state_len %d (1..5)"
                         % (Lmax + 1 - state_len, state_len))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    logz = torch.empty(N, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.bh_crf_seq_logz_grad(_lib.ptr(scores), N, T, state_len, five, float(blank_score or 0.0), s_n, s_t,
                                            _lib.ptr(targets), Lmax, targets.element_size(), _lib.ptr(lengths), _lib.ptr(weight),
                                            _lib.ptr(ws), _lib.ptr(logz), _lib.ptr(out), g_n, g_t, g32, int(bool(accumulate)),
                                            _lib.stream_ptr(dev)), "bh_crf_seq_logz_grad")
    return logz, out


def logz_grad(scores, state_len, blank_score=None, weight=None, out=None):
    """CTC_CRF.logZ AND its gradient from one launch (bh_crf_logz_dense_grad): (logZ float32 [N], grad), both on the device.
    grad[n, t, :] = weight[n] * the posterior probability of every edge at step t (SequenceDist.posteriors with the Log semiring);
    shape and dtype of `scores` (either layout; the koi layout has the four move edges per state only), or written into ``out``.
    Every element is written; fp32 scores are rounded to fp16 for the kernel."""
    state_len = int(state_len)
    scores, gdtype = _grad_scores(scores, state_len, blank_score)
    N, T, five, s_n, s_t = seq_layout(scores, state_len, blank_score)
    out, g_n, g_t, g32 = _grad_out(out, scores, gdtype, state_len, blank_score)
    lib = _lib.lib()
    dev = scores.device
    weight = _weight(weight, N, dev)
    nbytes = lib.bh_crf_logz_dense_grad_workspace(N, T, state_len)
    if nbytes == 0:
        raise ValueError("unsupported shape: N %d, T %d, state_len %d (1..5)" % (N, T, state_len))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    logz = torch.empty(N, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.bh_crf_logz_dense_grad(_lib.ptr(scores), N, T, state_len, five, float(blank_score or 0.0), s_n, s_t,
                                              _lib.ptr(weight), _lib.ptr(ws), _lib.ptr(logz), _lib.ptr(out), g_n, g_t, g32,
                                              _lib.stream_ptr(dev)), "bh_crf_logz_dense_grad")
    return logz, out


def encode_sequences(sequences):
    """Strings over ACGT, or a decoder's int8 plane [N, T] (ASCII bases, 0 = nothing emitted: beam_search's `sequence`,
    path_to_sequence's output) -> (targets int8 [N, Lmax] with labels 1..4 and 0 padding, lengths int32 [N]), CPU tensors."""
    lut = np.zeros(256, np.int8)
    lut[np.frombuffer(b"ACGT", np.uint8)] = (1, 2, 3, 4)
    if isinstance(sequences, (torch.Tensor, np.ndarray)):
        plane = sequences.cpu().numpy() if isinstance(sequences, torch.Tensor) else sequences
        rows = [r[r != 0].astype(np.uint8) for r in plane]
    else:
        rows = [np.frombuffer(s.encode() if isinstance(s, str) else bytes(s), np.uint8) for s in sequences]
    Lmax = max([len(r) for r in rows] + [1])
    targets = np.zeros((len(rows), Lmax), np.int8)
    for i, r in enumerate(rows):
        lab = lut[r]
        if (lab == 0).any():
            raise ValueError("sequence %d holds bytes outside ACGT" % i)
        targets[i, :len(r)] = lab
    return torch.from_numpy(targets), torch.tensor([len(r) for r in rows], dtype=torch.int32)


def seq_logprob(scores, sequences, blank_score=2.0):
    """ln P(sequence | scores) per chunk of koi-layout scores cuda fp16 [N, T, 4S] -> CPU float64 [N]: the model's exact sequence
    likelihood (what oracle.crf_ref.seq_logprob computes on the CPU), a decoder-independent figure for any called sequence.
    Built as  bh_crf_seq_logz_free - bh_crf_logz:  the numerator sums over every alignment of the sequence AND every start
    state (the loss's chain fixes the first k-mer instead; the free start has a kernel entry of its own)."""
    sl = state_len_of(scores.shape[-1])
    targets, lengths = encode_sequences(sequences)
    num = seq_logz(scores, targets, lengths, sl, blank_score, free_start=True)
    den = logz_any(scores, sl, blank_score)
    return (num.double() - den).cpu()


# ---- the CTC loss of bonito.ctc (csrc/ctc_loss.hip) -------------------------------------------------------------------------------------
# bytes of alpha workspace per launch of ctc_nll_grad: T x (2 Lmax + 1) x 4 bytes per chunk, 1.85 GB for 256 chunks of bonito.ctc's training
# shape (T = 1334, targets up to 675), which one launch should hold: a chunk is a workgroup, and half a batch leaves half the device idle
CTC_WORKSPACE_BUDGET = 4 << 30


def _ctc_args(log_probs, targets, lengths, weights, layout):
    """Checks and views shared by ctc_nll / ctc_nll_grad -> (log_probs, tnc, T, N, C, targets, lengths, weights)."""
    if log_probs.dim() != 3:
        raise ValueError("log_probs must be [T, N, C] or [N, T, C], got shape %s" % (tuple(log_probs.shape),))
    if targets.dim() != 2 or lengths.dim() != 1 or targets.shape[0] != lengths.shape[0]:
        raise ValueError("targets must be [N, Lmax] and lengths [N]")
    N = int(targets.shape[0])
    if layout is None:
        layout = "TNC" if log_probs.shape[1] == N else "NTC"               # [T, N, C] (the reference's) wins where both fit
    if layout not in ("TNC", "NTC"):
        raise ValueError("layout must be 'TNC' or 'NTC'")
    tnc = layout == "TNC"
    if log_probs.shape[1 if tnc else 0] != N:
        raise ValueError("%d target rows for log_probs of shape %s (%s)" % (N, tuple(log_probs.shape), layout))
    T, C = int(log_probs.shape[0 if tnc else 1]), int(log_probs.shape[2])
    if not 2 <= C <= 8:
        raise ValueError("the CTC loss kernel takes 2..8 classes, got %d" % C)
    if N < 1 or T < 1:
        raise ValueError("empty problem: N %d, T %d" % (N, T))
    if targets.shape[1] > 2047:
        raise ValueError("target rows of %d labels exceed the supported 2047" % targets.shape[1])
    if targets.dtype.is_floating_point or lengths.dtype.is_floating_point:
        raise TypeError("targets and lengths must be integers")
    if not log_probs.is_cuda:
        raise _lib.HipEngineError("log_probs must live on a HIP device (no CPU fallback)")
    if log_probs.dtype not in (torch.float16, torch.float32):
        raise TypeError("log_probs must be fp16 or fp32, got %s" % log_probs.dtype)
    if not lengths.is_cuda:                                                # host lengths are checked here; device lengths by the kernel (NaN)
        lo, hi = int(lengths.min()), int(lengths.max())
        if lo < 0 or hi > targets.shape[1]:
            raise ValueError("target lengths must lie in 0..%d (got %d..%d)" % (targets.shape[1], lo, hi))
    dev = log_probs.device
    log_probs = log_probs.detach()
    if log_probs.stride(2) != 1:
        log_probs = log_probs.contiguous()
    if targets.dtype not in (torch.int8, torch.int32):
        targets = targets.to(torch.int32)
    targets = targets.to(dev).contiguous()
    lengths = lengths.to(device=dev, dtype=torch.int32).contiguous()
    if weights is not None:
        weights = torch.as_tensor(weights, dtype=torch.float32).detach().to(dev).contiguous()
        if weights.shape != (C,):
            raise ValueError("weights must be [C] = [%d]" % C)
    return log_probs, tnc, T, N, C, targets, lengths, weights


def _sub(t, lo, hi):
    return None if t is None else t[lo:hi]


def ctc_nll(log_probs, targets, lengths, weights=None, layout=None):
    """torch.nn.functional.ctc_loss(reduction='none') on the device (bh_ctc_loss), blank = class 0: (nll float32 [N], smooth).
    log_probs: device fp16 / fp32 [T, N, C] or [N, T, C] (`layout`; by default [T, N, C] when its second axis matches the targets), any
    strides with a dense class axis, fp32 read natively. targets [N, Lmax] int8 / int32 / int64 (labels 1..C-1, 0 = padding), lengths
    [N] on the host or the device. smooth[n] = sum_t sum_c weights[c] * log_probs[t, n, c] (None without `weights`). A target that
    cannot fit gives nll = +inf; a length outside 0..Lmax or a label outside 1..C-1 gives NaN."""
    if log_probs.requires_grad:
        from bonito_amd.nn import NoTorchCompute
        raise NoTorchCompute("this entry point returns plain tensors: for log_probs with requires_grad use Model.loss, which carries "
                             "the backward")
    lp, tnc, T, N, Cn, targets, lengths, weights = _ctc_args(log_probs, targets, lengths, weights, layout)
    lib = _lib.lib()
    dev = lp.device
    Lmax = int(targets.shape[1])
    s_t, s_n = (lp.stride(0), lp.stride(1)) if tnc else (lp.stride(1), lp.stride(0))
    ws = torch.empty(lib.bh_ctc_loss_workspace(N, T, Cn, Lmax), dtype=torch.uint8, device=dev)
    nll = torch.empty(N, dtype=torch.float32, device=dev)
    smooth = torch.empty(N, dtype=torch.float32, device=dev) if weights is not None else None
    with torch.cuda.device(dev):
        _lib.check(lib.bh_ctc_loss(_lib.ptr(lp), int(lp.dtype == torch.float32), N, T, Cn, s_t, s_n, _lib.ptr(targets) if Lmax else None,
                                   Lmax, targets.element_size(), _lib.ptr(lengths), _lib.ptr(weights), _lib.ptr(ws), _lib.ptr(nll),
                                   _lib.ptr(smooth), _lib.stream_ptr(dev)), "bh_ctc_loss")
    return nll, smooth


def ctc_nll_grad(log_probs, targets, lengths, weights=None, weight=None, smooth_weight=None, out=None, accumulate=False, layout=None,
                 workspace_budget=None):
    """ctc_nll AND its gradient from one launch per group of chunks (bh_ctc_loss_grad): (nll, smooth, grad), all on the device.
    grad[t, n, c] (+)= -weight[n] * occ[t, c] + smooth_weight[n] * weights[c], where occ is the posterior probability that the path
    is, at step t, in a state of class c. THIS IS THE TRUE DERIVATIVE of nll with respect to log_probs; torch's native ctc_loss
    backward returns exp(log_probs) - occ instead, the derivative with respect to the logits in front of a log_softmax, and the two
    are identical after log_softmax's backward (g - exp(lp) * sum_c g). grad has the shape and dtype of `log_probs`, or is written
    into ``out`` (fp16 / fp32, same shape, own strides, dense class axis); ``accumulate=True`` adds into it. A chunk whose target
    cannot fit has nll = +inf and a ZERO gradient (this project's definition; torch gives NaN). The N chunks are split into groups
    whose alpha workspace (T x (2 Lmax + 1) x 4 bytes per chunk) stays under ``workspace_budget`` bytes (CTC_WORKSPACE_BUDGET); every
    chunk is computed by itself, so the result does not depend on the split, and it is bit-identical from call to call."""
    lp, tnc, T, N, Cn, targets, lengths, weights = _ctc_args(log_probs, targets, lengths, weights, layout)
    if accumulate and out is None:
        raise ValueError("accumulate=True needs out")
    if smooth_weight is not None and weights is None:
        raise ValueError("smooth_weight needs weights")
    dev = lp.device
    if out is None:
        out = torch.empty(lp.shape, dtype=lp.dtype, device=dev)
    else:
        if tuple(out.shape) != tuple(lp.shape) or out.device != dev:
            raise ValueError("out must have the shape %s and the device of log_probs" % (tuple(lp.shape),))
        if out.dtype not in (torch.float16, torch.float32):
            raise TypeError("out must be fp16 or fp32, got %s" % out.dtype)
        if out.stride(2) != 1:
            raise ValueError("the class axis of out must be dense")
        if out.requires_grad:
            raise ValueError("out must not require grad")
    weight, smooth_weight = _weight(weight, N, dev), _weight(smooth_weight, N, dev)
    lib = _lib.lib()
    Lmax = int(targets.shape[1])
    s_t, s_n = (lp.stride(0), lp.stride(1)) if tnc else (lp.stride(1), lp.stride(0))
    g_t, g_n = (out.stride(0), out.stride(1)) if tnc else (out.stride(1), out.stride(0))
    budget = CTC_WORKSPACE_BUDGET if workspace_budget is None else int(workspace_budget)
    per = lib.bh_ctc_loss_grad_workspace(1, T, Cn, Lmax) - 512
    group = max(1, min(N, budget // max(per, 1)))
    ws = torch.empty(lib.bh_ctc_loss_grad_workspace(group, T, Cn, Lmax), dtype=torch.uint8, device=dev)
    nll = torch.empty(N, dtype=torch.float32, device=dev)
    smooth = torch.empty(N, dtype=torch.float32, device=dev) if weights is not None else None
    esz, gsz = lp.element_size(), out.element_size()
    with torch.cuda.device(dev):
        st = _lib.stream_ptr(dev)
        for lo in range(0, N, group):
            hi = min(N, lo + group)
            _lib.check(lib.bh_ctc_loss_grad(
                C.c_void_p(lp.data_ptr() + lo * s_n * esz), int(lp.dtype == torch.float32), hi - lo, T, Cn, s_t, s_n,
                _lib.ptr(targets[lo:hi]) if Lmax else None, Lmax, targets.element_size(), _lib.ptr(lengths[lo:hi]), _lib.ptr(weights),
                _lib.ptr(_sub(weight, lo, hi)), _lib.ptr(_sub(smooth_weight, lo, hi)), _lib.ptr(ws), _lib.ptr(nll[lo:hi]),
                _lib.ptr(_sub(smooth, lo, hi)), C.c_void_p(out.data_ptr() + lo * g_n * gsz), g_t, g_n, int(out.dtype == torch.float32),
                int(bool(accumulate)), st), "bh_ctc_loss_grad")
    return nll, smooth, out

"""The CTC head, the two CTC decoders and the residual RMSNorm, each kernel alone against its reference (run with -m gpu on MI355X).

References: tests/ctc_kernels_ref.py (fp64 numpy, with the tolerance each element is allowed) for bh_ctc_head and bh_rmsnorm_residual;
oracle/ctc_ref.py for bh_ctc_greedy_decode (sequence, path and count exact, q-strings next to a rounding boundary only) and
bh_ctc_beam_search (labels, paths and counts bit for bit). Every output buffer - and the prefix beam's workspace, of exactly
bh_ctc_beam_search_workspace bytes - sits between 4 KiB guards of 0xA5 that are checked after the call, and so is every entry inside an
output that the kernel must not write (behind count[r] in a read's segment).

Launch geometries of the prefix beam (lanes = reads per workgroup, restated by ctc_kernels_ref.beam_lanes): (5, 5), (2, 1), (3, 2) run
with 64 lanes, (5, 8) with 32, (5, 16) and (8, 16) with 16; each pair with R = 1, L - 1, L (one workgroup), L + 1 (a second workgroup of
one read) and 2 L + 2 (three workgroups, the last of two reads).

Measured on MI355X (printed by the last test of this file):
  ctc_head           worst |d| / tol 0.995 (|d| 1.95e-3 at classes = 8, F = 8, M = 255); the largest |d|, 5.5e-2, in the large-logit case
                     (classes = 5, F = 8: ratio 0.994). On every element of every case |d| lies inside the store and dot terms alone: the
                     unexplained deviation is 0, and so is the exp/log term, 4 x 0 (ctc_kernels_ref.HEAD_EXPLOG).
  rmsnorm_residual   worst |d| / tol 0.9974 (|d| 3.85e-3 at D = 1016, M = 1001, x given, alpha 1, eps 1e-5): the fp16 store at its half step.
  ctc_greedy         sequence, path and count equal in all 12 cases; 0 q characters differ from the oracle's.
  ctc_prefix_beam    labels, paths and counts equal in all 24 cases x 5 launches, the worst-fill and the permuted batch."""
import numpy as np
import pytest
import torch

import ctc_kernels_ref as kr
from bonito_amd import _lib
from bonito_amd.ctc import decode as ctc_decode
from oracle import ctc_ref

pytestmark = pytest.mark.gpu
GUARD = 4096
FILL = 0xA5
WORST = {}          # kernel -> (worst |d| / tol, worst |d|, worst unexplained |d|, case)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda", 0)


class Guarded:
    """`nbytes` device bytes between two guards, everything filled with 0xA5."""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = torch.full((2 * GUARD + self.n,), FILL, dtype=torch.uint8, device=dev())

    @property
    def ptr(self):
        import ctypes
        return ctypes.c_void_p(self.buf.data_ptr() + GUARD)

    def host(self, dtype):
        """The payload as a numpy array of `dtype`, after the guards were found intact."""
        h = self.buf.cpu().numpy()
        assert (h[:GUARD] == FILL).all(), "the guard in front of the buffer was written"
        assert (h[GUARD + self.n:] == FILL).all(), "the guard behind the buffer was written"
        return h[GUARD:GUARD + self.n].view(dtype)


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _note(kernel, ratio, d, excess, case):
    r, dd, ex, c = WORST.get(kernel, (-1.0, 0.0, 0.0, ""))
    WORST[kernel] = (ratio, d, max(ex, excess), case) if ratio > r else (r, dd, max(ex, excess), c)


# ---- CTC head -------------------------------------------------------------------------------------------------------------------
def _head(classes, F, M, large):
    x, w, b = kr.head_inputs(classes, F, M, large)
    ref, tol = kr.ctc_head(x, w, b)
    xd, wd, bd = _up(x), _up(w), _up(b)
    out = Guarded(M * classes * 2)
    _lib.check(_lib.lib().bh_ctc_head(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), out.ptr, M, F, classes, _lib.stream_ptr()), "bh_ctc_head")
    torch.cuda.synchronize()
    got = out.host(np.float16).reshape(M, classes).astype(np.float64)
    case = "classes=%d F=%d M=%d%s" % (classes, F, M, " large" if large else "")
    ok, ratio, d = kr.within(got, ref, tol)
    explained = kr.ctc_head(x, w, b, explog=0.0)[1]
    excess = float(np.nan_to_num(np.abs(got - ref) - explained, nan=np.inf).max())
    print("ctc_head %s: worst |d| %.3g, worst |d| / tol %.3f, worst |d| - (store + dot) %.3g" % (case, d, ratio, excess))
    _note("ctc_head", ratio, d, max(excess, 0.0), case)
    assert ok, "ctc_head %s: worst |d| / tol %.3f (|d| %.3g)" % (case, ratio, d)
    return got, ref, tol


@pytest.mark.parametrize("F", kr.HEAD_FEATURES)
@pytest.mark.parametrize("classes", kr.HEAD_CLASSES)
def test_ctc_head_against_fp64(classes, F):
    for M in kr.HEAD_ROWS:
        got, ref, tol = _head(classes, F, M, False)
        if classes == 1:
            assert not got.any(), "log_softmax over one class is exactly 0"
    # logits that reach about +-60: finite, and every row sums to 1 within what the element tolerances allow
    got, ref, tol = _head(classes, F, kr.HEAD_ROWS[-1], True)
    assert np.isfinite(got).all()
    assert (np.abs(np.exp(got).sum(axis=-1) - 1.0) <= kr.head_row_sum_tolerance(ref, tol)).all()
    if classes == 1:
        assert not got.any()


# ---- RMSNorm --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", kr.NORM_M)
@pytest.mark.parametrize("D", kr.NORM_D)
def test_rmsnorm_residual_against_fp64(D, M):
    a, x, w = kr.norm_inputs(D, M)
    ad, xd, wd = _up(a), _up(x), _up(w)
    for with_x in (True, False):
        for alpha in kr.NORM_ALPHA:
            for eps in kr.NORM_EPS:
                ref, tol = kr.rmsnorm_residual(a, x if with_x else None, w, alpha, eps)
                out = Guarded(M * D * 2)
                _lib.check(_lib.lib().bh_rmsnorm_residual(_lib.ptr(ad), _lib.ptr(xd) if with_x else None, _lib.ptr(wd), out.ptr, M, D, alpha,
                                                          eps, _lib.stream_ptr()), "bh_rmsnorm_residual")
                torch.cuda.synchronize()
                got = out.host(np.float16).reshape(M, D).astype(np.float64)
                case = "D=%d M=%d x=%s alpha=%g eps=%g" % (D, M, "given" if with_x else "NULL", alpha, eps)
                ok, ratio, d = kr.within(got, ref, tol)
                _note("rmsnorm_residual", ratio, d, 0.0, case)
                assert ok, "rmsnorm_residual %s: worst |d| / tol %.3f (|d| %.3g)" % (case, ratio, d)
                if M >= 3:
                    assert not got[0].any(), "a row of zeros must give zeros"
                    assert np.isfinite(got[1]).all() and np.abs(got[1]).max() > 0.5       # |values| near 6e4: fp32 statistics hold them
    print("rmsnorm_residual D=%d M=%d: worst so far %r" % (D, M, WORST["rmsnorm_residual"]))


# ---- greedy decode --------------------------------------------------------------------------------------------------------------
_GREEDY = {}


def _greedy_case(C, qscale, qbias):
    """The reads of kr.greedy_reads(C) and the oracle's answer for each, computed once per (classes, qscale, qbias)."""
    key = (C, qscale, qbias)
    if key not in _GREEDY:
        reads = _GREEDY.setdefault(("reads", C), kr.greedy_reads(C))
        _GREEDY[key] = (reads, [ctc_ref.viterbi_search(lp, kr.ALPHABET[:C], qscale, qbias, return_qfloat=True) for lp in reads])
    return _GREEDY[key]


def _greedy_abi(reads, C, qscale, qbias):
    lens = [len(r) for r in reads]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total, R = int(offs[-1]), len(reads)
    flat = _up(np.concatenate(reads).astype(np.float32).reshape(total, C))
    offs_d = _up(offs)
    lab, qual, path, cnt = Guarded(total), Guarded(total), Guarded(4 * total), Guarded(4 * R)
    _lib.check(_lib.lib().bh_ctc_greedy_decode(_lib.ptr(flat), _lib.ptr(offs_d), R, C, qscale, qbias, lab.ptr, qual.ptr, path.ptr, cnt.ptr,
                                               _lib.stream_ptr()), "bh_ctc_greedy_decode")
    torch.cuda.synchronize()
    return offs, lab.host(np.uint8), qual.host(np.uint8), path.host(np.uint32), cnt.host(np.int32)


@pytest.mark.parametrize("qscale,qbias", kr.GREEDY_QPARAMS)
@pytest.mark.parametrize("C", kr.GREEDY_CLASSES)
def test_greedy_decode_against_the_oracle(C, qscale, qbias):
    reads, want = _greedy_case(C, qscale, qbias)
    letters = np.frombuffer(kr.ALPHABET.encode(), dtype=np.uint8)
    flips = 0
    for R in (1, 2, 70):
        offs, lab, qual, path, cnt = _greedy_abi(reads[:R], C, qscale, qbias)
        qs_all, oqs_all, oqf_all = [], [], []
        for r in range(R):
            oseq, oqs, opath, oqf = want[r]
            o, n, T = int(offs[r]), int(cnt[r]), len(reads[r])
            assert n == len(oseq), "read %d of %d (T = %d): %d bases, the oracle has %d" % (r, R, T, n, len(oseq))
            assert letters[lab[o:o + n]].tobytes().decode() == oseq, (r, R, T)
            assert path[o:o + n].tolist() == opath, (r, R, T)
            # behind count[r] the read's segment keeps the fill pattern
            assert (lab[o + n:o + T] == FILL).all() and (qual[o + n:o + T] == FILL).all() and (path[o + n:o + T] == 0xA5A5A5A5).all(), (r, R, T)
            qs_all.append(qual[o:o + n])
            oqs_all.append(np.frombuffer(oqs.encode("latin-1"), dtype=np.uint8))
            oqf_all.append(oqf)
        flips += kr.assert_greedy_qstrings(np.concatenate(qs_all), np.concatenate(oqs_all), np.concatenate(oqf_all), qscale, qbias)
    # the planted pair: read 0's last run reaches its last step, read 1 starts with the same label and emits at step 0
    assert want[0][2][-1] == len(reads[0]) - 2 and want[1][2][0] == 0 and want[0][0][-1] == want[1][0][0] == kr.ALPHABET[1]
    print("ctc_greedy classes=%d qscale=%g qbias=%g: %d q characters differ from the oracle's (each next to a rounding boundary)" % (C, qscale, qbias, flips))


def test_greedy_decode_through_the_python_surface():
    C, (qscale, qbias) = 5, kr.GREEDY_QPARAMS[1]
    reads, want = _greedy_case(C, qscale, qbias)
    got = ctc_decode.viterbi_search_batch([torch.from_numpy(r) for r in reads], kr.ALPHABET[:C], qscale, qbias)
    assert len(got) == len(reads)
    for (seq, qs, path), (oseq, oqs, opath, oqf) in zip(got, want):
        assert seq == oseq and path == opath
        kr.assert_greedy_qstrings(qs, oqs, oqf, qscale, qbias)
    # reads that are all empty: empty results, no null pointer handed to the library
    empty = [torch.zeros(0, C), torch.zeros(0, C), torch.zeros(0, C)]
    assert ctc_decode.viterbi_search_batch(empty, kr.ALPHABET[:C]) == [("", "", [])] * 3
    assert ctc_decode.beam_search_batch(empty, kr.ALPHABET[:C]) == [("", [])] * 3
    # ... and an empty read among others is an empty result in its place
    mixed = ctc_decode.viterbi_search_batch([torch.zeros(0, C), torch.from_numpy(reads[1]), torch.zeros(0, C)], kr.ALPHABET[:C], qscale, qbias)
    assert mixed[0] == mixed[2] == ("", "", []) and mixed[1][0] == want[1][0] and mixed[1][2] == want[1][2]


# ---- prefix beam ----------------------------------------------------------------------------------------------------------------
def _beam_abi(reads, C, B, thr):
    lens = [len(r) for r in reads]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total, R = int(offs[-1]), len(reads)
    flat = _up(np.concatenate(reads).astype(np.float32).reshape(total, C))
    offs_d = _up(offs)
    ws = Guarded(_lib.lib().bh_ctc_beam_search_workspace(total, R, C, B))
    lab, path, cnt = Guarded(total), Guarded(4 * total), Guarded(4 * R)
    _lib.check(_lib.lib().bh_ctc_beam_search(_lib.ptr(flat), _lib.ptr(offs_d), R, C, B, thr, ws.ptr, lab.ptr, path.ptr, cnt.ptr,
                                             _lib.stream_ptr()), "bh_ctc_beam_search")
    torch.cuda.synchronize()
    ws.host(np.uint8)
    lab, path, cnt = lab.host(np.uint8), path.host(np.uint32), cnt.host(np.int32)
    letters = np.frombuffer(kr.ALPHABET.encode(), dtype=np.uint8)
    out = []
    for r in range(R):
        o, n, T = int(offs[r]), int(cnt[r]), lens[r]
        assert 0 <= n <= T, (r, n, T)
        assert (lab[o + n:o + T] == FILL).all() and (path[o + n:o + T] == 0xA5A5A5A5).all(), "read %d: written behind count" % r
        out.append((letters[lab[o:o + n]].tobytes().decode(), path[o:o + n].tolist()))
    return out


def _beam_check(reads, want, C, B, thr, R):
    got = _beam_abi(reads[:R], C, B, thr)
    for r in range(R):
        assert got[r] == want[r], "classes=%d beam=%d threshold=%g R=%d read %d (T = %d): %d bases, the oracle has %d" % (
            C, B, thr, R, r, len(reads[r]), len(got[r][0]), len(want[r][0]))


@pytest.mark.parametrize("thr", kr.BEAM_THRESHOLDS)
@pytest.mark.parametrize("C,B", kr.BEAM_PAIRS)
def test_prefix_beam_against_the_oracle(C, B, thr):
    L = kr.beam_lanes(C, B)
    reads = kr.beam_reads(C, 2 * L + 2)
    want = [ctc_ref.beam_search(lp, kr.ALPHABET[:C], B, thr) for lp in reads]
    for R in sorted({1, L - 1, L, L + 1, 2 * L + 2}):
        _beam_check(reads, want, C, B, thr, R)
    if thr == 0.999:
        # a read none of whose labels ever reaches p = 0.999 decodes to nothing (the sharpest reads do hold such steps)
        quiet = [bool((lp[:, 1:] < np.float32(np.log(np.float32(0.999)))).all()) for lp in reads]
        assert sum(quiet) > len(reads) // 2 and all(w == ("", []) for w, q in zip(want, quiet) if q)
    elif thr > 1e-4:
        assert want[4] == ("", []) and any(w[0] for w in want), "the read whose beam empties decodes to nothing"
    print("ctc_prefix_beam classes=%d beam=%d threshold=%g: %d lanes per workgroup, launches of %s workgroups; %d bases" % (
        C, B, thr, L, sorted({(R + L - 1) // L for R in (1, L - 1, L, L + 1, 2 * L + 2)}), sum(len(w[0]) for w in want)))


def test_prefix_beam_worst_fill():
    """Threshold 0 at the widest search (8 classes, beam 16), 17 reads in two workgroups: near-flat rows, whose steps hold all B * C = 128
    candidates, and forking rows, which allocate B new nodes per step (the pool's bound); tests/test_ctc_kernels_ref_cpu.py counts both on
    these reads. A write past either array lands in a neighbouring lane's LDS, a neighbouring read's nodes or the workspace guard."""
    C, B, T = 8, 16, 50
    L = kr.beam_lanes(C, B)
    reads = kr.beam_reads(C, L + 1, flat=True, T=T)
    want = [ctc_ref.beam_search(lp, kr.ALPHABET[:C], B, 0.0) for lp in reads]
    _beam_check(reads, want, C, B, 0.0, L + 1)


def test_prefix_beam_permuted_batch():
    C, B, thr = 5, 8, 1e-3
    L = kr.beam_lanes(C, B)
    reads = kr.beam_reads(C, 2 * L + 2)
    perm = np.random.default_rng(5).permutation(len(reads))
    assert (perm != np.arange(len(reads))).sum() > L
    plain = _beam_abi(reads, C, B, thr)
    mixed = _beam_abi([reads[i] for i in perm], C, B, thr)
    assert [plain[i] for i in perm] == mixed
    via = ctc_decode.beam_search_batch([torch.from_numpy(reads[i]) for i in perm], kr.ALPHABET[:C], B, thr)
    assert via == mixed


def test_zz_report_the_worst_deviation_per_kernel():
    """Not a check of its own: prints what the tests above measured (run the whole file with -s to see it)."""
    for kernel, (ratio, d, excess, case) in sorted(WORST.items()):
        print("%s: worst |d| / tol %.4f (|d| %.4g, unexplained by the derived terms %.3g) at %s" % (kernel, ratio, d, excess, case))

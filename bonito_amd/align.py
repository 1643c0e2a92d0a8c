"""
Pairwise local alignment on the device: the engine's counterpart of ``parasail.sw_trace_striped_32(seq, ref, 8, 4, dnafull)``, the one
call behind the reference's read accuracy (bonito/cli/evaluate.py:37-67 ``align``, bonito/util.py:346-368 ``accuracy``).

``sw_align`` is the batched entry (kernel: csrc/align.hip through ``bh_sw_align``); ``align`` / ``AlignResult`` carry the reference's
names. The definition, with its tie-breaks, is in DESIGN.md section 6. There is no host fallback.

The duplex caller's two alignments live here too: ``sg_align`` (the semi-global mode of the same kernels, ``bh_sg_align``; parasail's
``sg_trace_scan_32``) and ``nw_align`` (banded global alignment under unit costs for reads of up to 65536 bases, csrc/nw.hip through
``bh_nw_align``; edlib's ``align(..., task="path")``), bonito/cli/duplex.py:224-269.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from bonito_amd import _lib
from bonito_amd.decode import encode_sequences

OPS = "=XID"                                     # op codes of bh_sw_align's runs: (length << 2) | op
MAX_LEN = 4096
# Traceback bits cost ceil(seq / 512) * (ref + 63) * 256 bytes per pair (8.1 MiB at 4096 x 4096, 0.42 MiB for a 10 000-sample chunk's
# ~ 800 bases). 1 GiB holds 126 pairs of the largest size or about 2 400 chunks in one launch, and stays small beside the 288 GB card.
DEFAULT_WORKSPACE_BUDGET = 1 << 30
COLUMNS = ("score", "num_correct", "num_mismatches", "num_insertions", "num_deletions",
           "align_ref_start", "align_ref_end", "align_seq_start", "align_seq_end", "num_runs")


@dataclass
class AlignResult:
    """One pair; the reference's fields (cli/evaluate.py:22-34) plus the score and, when asked for, the CIGAR. A pair with nothing
    in common (score 0, an empty sequence among them) has counts 0, starts 0, ends -1, an empty CIGAR and accuracy 0."""
    accuracy: float = 0
    num_correct: int = 0
    num_mismatches: int = 0
    num_insertions: int = 0
    num_deletions: int = 0
    ref_len: int = 0
    seq_len: int = 0
    align_ref_start: int = 0
    align_ref_end: int = -1
    align_seq_start: int = 0
    align_seq_end: int = -1
    score: int = 0
    cigar: str = None


def accuracy_of(num_correct, num_mismatches, num_insertions, num_deletions):
    """num_correct / (all alignment columns), 0 where nothing aligned; arrays or scalars."""
    c = np.asarray(num_correct, np.float64)
    total = c + np.asarray(num_mismatches) + np.asarray(num_insertions) + np.asarray(num_deletions)
    return np.divide(c, total, out=np.zeros_like(total, dtype=np.float64), where=total > 0)


class _Batch:
    """What ``SwBatch`` and ``NwBatch`` share: ``table`` int32 [n, len(columns)], ``seq_len`` / ``ref_len``, every column an attribute."""
    columns = ()

    def __init__(self, table, seq_len, ref_len):
        self.table = np.asarray(table, np.int32).reshape(-1, len(self.columns))
        self.seq_len = np.asarray(seq_len, np.int32)
        self.ref_len = np.asarray(ref_len, np.int32)

    def __len__(self):
        return self.table.shape[0]

    def __getattr__(self, name):
        if name in self.columns:
            return self.table[:, self.columns.index(name)]
        raise AttributeError(name)


class SwBatch(_Batch):
    """Results of one ``sw_align`` call in the caller's order: ``table`` int32 [n, 10] (``COLUMNS``), ``seq_len`` / ``ref_len``,
    ``cigar`` (list of strings, or None); every column is an attribute, ``batch[i]`` is an ``AlignResult``."""
    columns = COLUMNS

    def __init__(self, table, seq_len, ref_len, cigar=None):
        super().__init__(table, seq_len, ref_len)
        self.cigar = cigar

    @property
    def accuracy(self):
        return accuracy_of(self.num_correct, self.num_mismatches, self.num_insertions, self.num_deletions)

    def __getitem__(self, i):
        row = [int(v) for v in self.table[i]]
        return AlignResult(
            accuracy=float(accuracy_of(*row[1:5])), num_correct=row[1], num_mismatches=row[2], num_insertions=row[3],
            num_deletions=row[4], ref_len=int(self.ref_len[i]), seq_len=int(self.seq_len[i]), align_ref_start=row[5],
            align_ref_end=row[6], align_seq_start=row[7], align_seq_end=row[8], score=row[0],
            cigar=None if self.cigar is None else self.cigar[i])


def runs_to_cigar(runs):
    """uint32 runs of bh_sw_align -> '12=1X3=...'."""
    return "".join("%d%s" % (int(r) >> 2, OPS[int(r) & 3]) for r in runs)


def _encode(x, what):
    """strings / an ASCII plane (decode.encode_sequences) or a code plane (integers 0..4, 0 = padding after the bases)
    -> (int8 codes [n, L] CPU tensor, int32 lengths numpy)."""
    if isinstance(x, (torch.Tensor, np.ndarray)):
        plane = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
        if plane.ndim != 2:
            raise ValueError("%s: a plane must be [n, L]" % what)
        if plane.size == 0 or int(plane.max()) <= 4:
            if plane.size and int(plane.min()) < 0:
                raise ValueError("%s: codes must be 0..4" % what)
            lens = (plane != 0).sum(axis=1).astype(np.int32)
            if ((plane != 0) != (np.arange(plane.shape[1])[None, :] < lens[:, None])).any():
                raise ValueError("%s: padding (0) inside a row of codes" % what)
            return torch.from_numpy(np.ascontiguousarray(plane.astype(np.int8))), lens
    codes, lens = encode_sequences(x)
    return codes, lens.numpy().astype(np.int32)


def _slices(order, seq_len, ref_len, band, budget, workspace):
    """Cut the size-sorted pairs into runs whose workspace(count, max seq, max ref, max band) stays within the budget -> (runs of
    (indices, max seq, max ref, max band), indices of the pairs that do not fit alone)."""
    out, unfit, lo = [], [], 0
    while lo < len(order):
        hi, ms, mr, mb = lo, 0, 0, 1
        while hi < len(order):
            i = order[hi]
            s, r, b = max(ms, int(seq_len[i])), max(mr, int(ref_len[i])), max(mb, int(band[i]))
            if workspace(hi - lo + 1, s, r, b) > budget:
                break
            hi, ms, mr, mb = hi + 1, s, r, b
        if hi == lo:
            unfit.append(order[lo])
            lo += 1
            continue
        out.append((order[lo:hi], ms, mr, mb))
        lo = hi
    return out, unfit


def _launch(entry, extra, nbytes, width, codes, lens, idx, ms, mr, need, device):
    """One launch of the entry point named ``entry`` over the pairs ``idx`` (maxima ms, mr; ``extra``: its arguments between the pair
    count and the workspace of ``nbytes`` bytes; ``need``: per pair the most CIGAR runs, or None for no CIGAR) -> (the int32 result
    rows [len(idx), width], per pair its uint32 runs - views of one plane cut to the widest count - or None)."""
    k = len(idx)
    sel = torch.from_numpy(np.ascontiguousarray(idx))
    s_dev = codes[0][sel][:, :max(ms, 1)].contiguous().to(device)
    r_dev = codes[1][sel][:, :max(mr, 1)].contiguous().to(device)
    s_len, r_len = np.ascontiguousarray(lens[0][idx]), np.ascontiguousarray(lens[1][idx])
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    res = torch.empty((k, width), dtype=torch.int32, device=device)
    ops = n_ops = None
    stride = 0
    if need is not None:
        stride = max(1, int(need[idx].max()))
        ops = torch.empty((k, stride), dtype=torch.int32, device=device)
        n_ops = torch.empty(k, dtype=torch.int32, device=device)
    ip = C.POINTER(C.c_int32)
    _lib.check(getattr(_lib.lib(), entry)(_lib.ptr(s_dev), s_dev.shape[1], s_len.ctypes.data_as(ip), _lib.ptr(r_dev), r_dev.shape[1],
                                          r_len.ctypes.data_as(ip), k, *extra, _lib.ptr(ws), nbytes, _lib.ptr(res), _lib.ptr(ops),
                                          stride, _lib.ptr(n_ops), _lib.stream_ptr(s_dev.device)), entry)
    rows = res.cpu().numpy()
    if need is None:
        return rows, None
    counts = n_ops.cpu().numpy()
    plane = ops[:, :max(int(counts.max()), 1)].cpu().numpy().view(np.uint32)
    return rows, [plane[row, :counts[row]] for row in range(k)]


def sw_align(seqs, refs, match=5, mismatch=-4, gap_open=8, gap_extend=4, cigar=False, workspace_budget=DEFAULT_WORKSPACE_BUDGET,
             device="cuda"):
    """Smith-Waterman with affine gaps (a gap of k costs gap_open + (k - 1) * gap_extend) of seqs[i] (the query) against refs[i], for
    lists of strings over ACGT (empty strings are legal) or code planes. The defaults are the reference's parasail arguments
    (dnafull on A, C, G, T: +5 / -4; open 8, extend 4). Pairs are sorted by size and cut into launches whose workspace stays within
    ``workspace_budget`` bytes; the results come back in the caller's order as a ``SwBatch``."""
    return _affine("sw_align", seqs, refs, match, mismatch, gap_open, gap_extend, cigar, workspace_budget, device)


def sg_align(seqs, refs, match=5, mismatch=-4, gap_open=10, gap_extend=2, cigar=True, workspace_budget=DEFAULT_WORKSPACE_BUDGET,
             device="cuda"):
    """The semi-global mode of the same aligner (kernel: ``bh_sg_align``): end gaps are free on both sequences at both ends, and the
    CIGAR covers both sequences completely - the unaligned head and tail come out as one I or D run each. The defaults are the
    reference's ``parasail.sg_trace_scan_32(query, ref, 10, 2, dnafull)`` (bonito/cli/duplex.py:240-243). The definition, with its
    tie-breaks, is in DESIGN.md section 6. Same limits, slicing and ``SwBatch`` as ``sw_align``; the counts include the overhang
    runs, the start / end columns describe the aligned part."""
    return _affine("sg_align", seqs, refs, match, mismatch, gap_open, gap_extend, cigar, workspace_budget, device)


def _affine(name, seqs, refs, match, mismatch, gap_open, gap_extend, cigar, workspace_budget, device):
    sg = name == "sg_align"
    sc, sl = _encode(seqs, "seqs")
    rc, rl = _encode(refs, "refs")
    n = len(sl)
    if len(rl) != n:
        raise ValueError("%s: %d seqs against %d refs" % (name, n, len(rl)))
    if max([0] + sl.tolist() + rl.tolist()) > MAX_LEN:
        raise ValueError("%s: sequences of up to %d bases are supported" % (name, MAX_LEN))
    table = np.zeros((n, len(COLUMNS)), np.int32)
    cigars = [""] * n if cigar else None
    if n == 0:
        return SwBatch(table, sl, rl, cigars)
    lib = _lib.lib()
    passes = (sl.astype(np.int64) + 511) // 512
    order = np.argsort(passes * (rl.astype(np.int64) + 63), kind="stable")
    slices, unfit = _slices(order, sl, rl, np.ones(n, np.int64), int(workspace_budget), lambda k, s, r, b: lib.bh_sw_workspace(k, s, r))
    if unfit:
        i = unfit[0]
        raise ValueError("sw_align: workspace_budget of %d bytes cannot hold one pair of lengths (%d, %d), which needs %d"
                         % (int(workspace_budget), sl[i], rl[i], lib.bh_sw_workspace(1, int(sl[i]), int(rl[i]))))
    need = None
    if cigar:
        need = sl + rl if sg else np.where((sl > 0) & (rl > 0), sl + rl - 1, 0)
    for idx, ms, mr, _ in slices:
        table[idx], runs = _launch("bh_sg_align" if sg else "bh_sw_align", (int(match), int(mismatch), int(gap_open), int(gap_extend)),
                                   lib.bh_sw_workspace(len(idx), ms, mr), len(COLUMNS), (sc, rc), (sl, rl), idx, ms, mr, need, device)
        if cigar:
            for i, r in zip(idx, runs):
                cigars[i] = runs_to_cigar(r)
    return SwBatch(table, sl, rl, cigars)


NW_COLUMNS = ("distance", "num_correct", "num_mismatches", "num_insertions", "num_deletions", "num_runs", "band", "status")
NW_MAX_LEN = 65536
NW_FIRST_BAND = 64                               # the first half-width k; a rejected pair runs again with k doubled ...
NW_MAX_BAND = 65536                              # ... up to the half-width at which the band holds every cell of the longest pair
# Traceback bits cost ceil(seq / 512) * (min(ref, 511 + band width) + 63) * 128 bytes per pair, band width = |ref - seq| + 2 k + 1:
# 4.3 MiB for 10 000 bases at k = 512, 60 MiB for 50 000 at k = 2048, 2 GiB for the full matrix of the longest pair. 8 GiB keeps a
# batch of 512 reads or 64 long ones in one launch, one wave per pair.
NW_WORKSPACE_BUDGET = 8 << 30
NW_OK, NW_NO_FIT = 0, 2                          # status: accepted / the band the pair needs does not fit the workspace budget


class NwBatch(_Batch):
    """Results of one ``nw_align`` call in the caller's order: ``table`` int32 [n, 8] (``NW_COLUMNS``), ``seq_len`` / ``ref_len``,
    ``runs`` (per pair the uint32 runs of bh_nw_align, or None; no runs where status is not 0), ``cigar`` (the same as strings, made
    on first use: long reads have thousands of runs each) and ``ops(i)`` (the same as [(length, op character)]); every column is an
    attribute."""
    columns = NW_COLUMNS

    def __init__(self, table, seq_len, ref_len, runs=None):
        super().__init__(table, seq_len, ref_len)
        self.runs = runs
        self._cigar = None

    @property
    def cigar(self):
        if self._cigar is None and self.runs is not None:
            self._cigar = [runs_to_cigar(r) for r in self.runs]
        return self._cigar

    def ops(self, i):
        r = self.runs[i]
        return list(zip((r >> 2).tolist(), [OPS[c] for c in (r & 3).tolist()]))


def nw_align(seqs, refs, cigar=True, band=NW_FIRST_BAND, workspace_budget=NW_WORKSPACE_BUDGET, device="cuda"):
    """Global alignment under unit costs (edit distance with a path) of seqs[i] (the query) against refs[i], for lists of strings
    over ACGT (empty strings are legal) or code planes of up to 65536 bases: the engine's counterpart of
    ``edlib.align(query, ref, task="path")`` (kernel: csrc/nw.hip through ``bh_nw_align``; the definition, its tie-breaks and the
    band argument are in DESIGN.md section 6). ``band`` is the first half-width k of the diagonal band; a pair whose banded distance
    d does not satisfy floor((d - |len difference|) / 2) <= k is run again with k doubled, so the results do not depend on it
    (except the column ``band``, the k that was accepted). Every round sorts its pairs by size and cuts them into launches whose
    workspace stays within ``workspace_budget`` bytes; a pair whose band does not fit the budget alone comes back with status
    ``NW_NO_FIT``, the last banded distance (an upper bound; -1 if none was computed) and no CIGAR. -> ``NwBatch``."""
    sc, sl = _encode(seqs, "seqs")
    rc, rl = _encode(refs, "refs")
    n = len(sl)
    if len(rl) != n:
        raise ValueError("nw_align: %d seqs against %d refs" % (n, len(rl)))
    if max([0] + sl.tolist() + rl.tolist()) > NW_MAX_LEN:
        raise ValueError("nw_align: sequences of up to %d bases are supported" % NW_MAX_LEN)
    k = int(band)
    if not 1 <= k <= NW_MAX_BAND:
        raise ValueError("nw_align: band must be in 1..%d" % NW_MAX_BAND)
    table = np.zeros((n, len(NW_COLUMNS)), np.int32)
    table[:, 0] = -1
    runs = [np.zeros(0, np.uint32)] * n if cigar else None
    if n == 0:
        return NwBatch(table, sl, rl, runs)
    lib = _lib.lib()
    need = sl + rl if cigar else None                                       # every op consumes a base
    todo = np.arange(n)
    while len(todo):
        band = np.abs(rl.astype(np.int64) - sl) + 2 * k + 1
        size = ((sl[todo].astype(np.int64) + 511) // 512) * np.minimum(rl[todo].astype(np.int64), 511 + band[todo])
        slices, unfit = _slices(todo[np.argsort(size, kind="stable")], sl, rl, band, int(workspace_budget), lib.bh_nw_workspace)
        for i in unfit:
            table[i, 1:] = (0, 0, 0, 0, 0, k, NW_NO_FIT)
        again = []
        for idx, ms, mr, mb in slices:
            rows, got = _launch("bh_nw_align", (k,), lib.bh_nw_workspace(len(idx), ms, mr, mb), len(NW_COLUMNS), (sc, rc), (sl, rl), idx,
                                ms, mr, need, device)
            table[idx] = rows
            if (rows[:, 7] > 1).any():
                raise RuntimeError("nw_align: the traceback left the band of an accepted pair")
            again.append(idx[rows[:, 7] == 1])
            if cigar:
                for i, r in zip(idx, got):
                    runs[i] = r.copy()
        todo = np.concatenate(again) if again else np.zeros(0, np.int64)
        if len(todo) and k >= NW_MAX_BAND:
            raise RuntimeError("nw_align: a pair was rejected at the largest band")       # the largest band holds every cell
        k = min(2 * k, NW_MAX_BAND)
    return NwBatch(table, sl, rl, runs)


def align(*, ref, seq, **scoring):
    """One pair with the reference's field names (bonito/cli/evaluate.py:37-67)."""
    return sw_align([seq], [ref], **scoring)[0]

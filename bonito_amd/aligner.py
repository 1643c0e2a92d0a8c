"""
Read mapping on the device: the engine's counterpart of ``mappy.Aligner`` and ``bonito.aligner.align_map`` behind
``bonito basecaller --reference`` (/root/reference bonito/aligner.py, bonito/cli/basecaller.py:73-76,139).

The mapper is DEFINED by the restatement tests/mapper_ref.py ("Mapper") and equals it bit for bit; it is not
minimap2: seeds, chain scores, mapq, tie-breaks and the missing drop-off extension at the ends all differ. Kernels: csrc/mapper.hip
(``bh_map_sketch``, ``bh_map_seed``, ``bh_map_chain``) and csrc/nw.hip through ``align.nw_align`` for the bases; sorting and prefix
sums are torch's. With ``extend_ends`` the alignment is carried beyond the outermost anchors by ``bh_map_extend`` (a banded
extension without drop-off, defined by tests/mapper_ext_ref.py); off by default, and then nothing changes. Spans and pieces are
numpy on the host; CIGAR merge, NM and MD are one host library call per read. There is no host fallback for the device steps.
"""
import ctypes as C
import gzip
import time

import numpy as np
import torch

from bonito_amd import _lib
from bonito_amd.align import nw_align

PIECE = 16384                                    # query bases per nw_align piece at most
MAX_READS = 1024                                 # reads per seed / chain call (the read index has 10 bits in an anchor word)
MAX_READ_LEN = (1 << 21) - 1
QBITS, RBITS = 21, 31
EXT_MAX, EXT_BAND = 512, 32                      # end extension: query bases per tail at most, the band's half-width
_LUT = np.full(256, 5, np.int8)                  # 1..4 = A C G T, 5 = any other byte
_LUT[np.frombuffer(b"ACGT", np.uint8)] = (1, 2, 3, 4)
_COMP = np.array([0, 4, 3, 2, 1, 5], np.int8)


class Mapping:
    """One primary alignment with mappy's field names (what io.sam_record / io.summary_row read). r_st / r_en and the CIGAR are on the
    reference strand, q_st / q_en on the read as given; cigar holds (count, op) with M / I / D = 0 / 1 / 2."""
    __slots__ = ("ctg", "r_st", "r_en", "q_st", "q_en", "strand", "mapq", "cigar", "cigar_str", "NM", "MD", "mlen", "blen")

    def __init__(self, **kw):
        for name in self.__slots__:
            setattr(self, name, kw[name])

    def as_dict(self):
        return {name: getattr(self, name) for name in self.__slots__}

    def __repr__(self):
        return "Mapping(%s)" % ", ".join("%s=%r" % (n, getattr(self, n)) for n in self.__slots__ if n != "cigar")


def read_fasta(path):
    """FASTA, plain or .gz -> [(name, SEQUENCE)]: names cut at the first whitespace, sequence upper-cased, line breaks joined."""
    opener = gzip.open if str(path).endswith(".gz") else open
    out, name, parts = [], None, []
    with opener(path, "rt") as fh:
        for line in fh:
            line = line.strip()
            if line.startswith(">"):
                if name is not None:
                    out.append((name, "".join(parts).upper()))
                fields = line[1:].split()
                name, parts = fields[0] if fields else "", []
            elif line and name is not None:
                parts.append(line)
    if name is not None:
        out.append((name, "".join(parts).upper()))
    return out


def encode(seq):
    return _LUT[np.frombuffer(seq.encode("latin-1"), np.uint8)]


def finish(runs, q, r, q_st, r_st):
    """The run words of nw_align for a read's pieces, in order, over the code arrays q (the read on the aligned strand) and r (the
    contig) from (q_st, r_st) -> (cigar [(count, op)] over M I D = 0 1 2 with equal neighbours merged, its text, NM, MD, mlen, blen);
    a column matches when both bases are the same base of ACGT. One host library call (``bh_host_map_finish``)."""
    runs = np.ascontiguousarray(runs, np.uint32)
    q, r = np.ascontiguousarray(q, np.int8), np.ascontiguousarray(r, np.int8)
    n = len(runs)
    cols = int((runs >> 2).sum())
    cigar = np.empty(max(n, 1), np.uint32)
    text, md = C.create_string_buffer(24 * (n + 2)), C.create_string_buffer(24 * (n + 2) + 2 * cols)
    counts = np.zeros(8, np.int64)
    rc = _lib.lib().bh_host_map_finish(runs.ctypes.data_as(C.c_void_p), n, q.ctypes.data_as(C.c_void_p), len(q), int(q_st),
                                       r.ctypes.data_as(C.c_void_p), len(r), int(r_st), cigar.ctypes.data_as(C.c_void_p), len(cigar),
                                       text, len(text), md, len(md), counts.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError("bh_host_map_finish failed (rc=%d)" % rc)
    nm, mlen, blen, n_cigar, n_text, n_md = (int(v) for v in counts[:6])
    words = cigar[:n_cigar]
    return (list(zip((words >> 2).tolist(), (words & 3).tolist())), text.raw[:n_text].decode("ascii"), nm,
            md.raw[:n_md].decode("ascii"), mlen, blen)


def span_and_pieces(rpos, qpos, k, q, r):
    """The chain's anchors (positions of the k-mers' last bases, increasing) on the aligned strand, code arrays q (the read) and r
    (the contig) -> (q_st, q_en, r_st, r_en, [(q0, q1, r0, r1)]): the span widened over equal bases, cut behind chain anchors into
    pieces of at most PIECE query bases."""
    r_st, q_st = int(rpos[0]) - k + 1, int(qpos[0]) - k + 1
    r_en, q_en = int(rpos[-1]) + 1, int(qpos[-1]) + 1
    while q_st > 0 and r_st > 0 and q[q_st - 1] == r[r_st - 1] and q[q_st - 1] < 5:
        q_st, r_st = q_st - 1, r_st - 1
    while q_en < len(q) and r_en < len(r) and q[q_en] == r[r_en] and q[q_en] < 5:
        q_en, r_en = q_en + 1, r_en + 1
    pieces, q0, r0 = [], q_st, r_st
    ends = qpos + 1
    while q_en - q0 > PIECE:
        x = int(np.searchsorted(ends, q0 + PIECE, side="right")) - 1     # the last anchor that keeps the piece within the limit
        if x < 0 or ends[x] <= q0:
            break                                                        # no anchor left to cut at: the last piece is longer
        pieces.append((q0, int(ends[x]), r0, int(rpos[x]) + 1))
        q0, r0 = int(ends[x]), int(rpos[x]) + 1
    pieces.append((q0, q_en, r0, r_en))
    return q_st, q_en, r_st, r_en, pieces


class Aligner:
    """``Aligner(reference.fasta)``: reads the contigs, sketches them on the device and keeps the sorted minimizer index and the
    reference codes resident there. ``map_batch(sequences)`` -> a ``Mapping`` or None per sequence."""

    def __init__(self, reference_path, k=15, w=10, max_occ=64, device="cuda", max_dist=5000, bandwidth=500, min_cnt=3, min_score=40,
                 extend_ends=False):
        if isinstance(reference_path, (list, tuple)):                                # contigs given directly: [(name, sequence)]
            contigs = [(str(n), str(s).upper()) for n, s in reference_path]
        elif str(reference_path).endswith(".mmi"):
            raise ValueError("%s: minimap2 index files (.mmi) are not supported; give the reference as FASTA (plain or .gz)"
                             % reference_path)
        if not 11 <= int(k) <= 28:
            raise ValueError("k must be in 11..28")
        if not 1 <= int(w) <= 64:
            raise ValueError("w must be in 1..64")
        self.k, self.w, self.max_occ, self.device = int(k), int(w), int(max_occ), device
        self.max_dist, self.bandwidth, self.min_cnt, self.min_score = int(max_dist), int(bandwidth), int(min_cnt), int(min_score)
        self.extend_ends = bool(extend_ends)
        self.timings = dict(sketch_seed=0.0, chain=0.0, base=0.0, host=0.0, extend=0.0)      # seconds, summed over map_batch calls
        self.set_contigs(contigs if isinstance(reference_path, (list, tuple)) else read_fasta(reference_path))

    def set_contigs(self, contigs):
        self.seq_names = [n for n, _ in contigs]
        self._seqs = dict(contigs)
        self._codes = [encode(s) for _, s in contigs]
        lens = np.array([len(c) for c in self._codes], np.int64)
        if lens.sum() >= 1 << 31:
            raise ValueError("the reference must be shorter than 2^31 bases")
        self._starts = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        if len(contigs) and lens.sum():
            self._build_index()

    def __bool__(self):
        return len(self.seq_names) > 0

    def seq(self, name, start=0, end=None):
        s = self._seqs.get(name)
        return None if s is None else s[start:end]

    # ---- device steps ------------------------------------------------------------------------------------------------------------

    def _sketch(self, codes, stride, lens):
        """DEVICE int8 codes ([n, stride], or one sequence) and numpy int32 lengths -> (keys, pos, strand, offsets) on the device"""
        lib = _lib.lib()
        n = len(lens)
        lens = np.ascontiguousarray(lens, np.int32)
        cap = max(1, int(np.maximum(lens.astype(np.int64) - self.k + 1, 0).sum()))
        nbytes = lib.bh_map_sketch_workspace(n, int(lens.astype(np.int64).sum()))
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=self.device)
        keys = torch.empty(cap, dtype=torch.int64, device=self.device)
        pos = torch.empty(cap, dtype=torch.int32, device=self.device)
        strand = torch.empty(cap, dtype=torch.int8, device=self.device)
        off = torch.empty(n + 1, dtype=torch.int32, device=self.device)
        _lib.check(lib.bh_map_sketch(_lib.ptr(codes), int(stride), lens.ctypes.data_as(C.c_void_p), n, self.k, self.w, _lib.ptr(ws),
                                     nbytes, _lib.ptr(keys), _lib.ptr(pos), _lib.ptr(strand), cap, _lib.ptr(off),
                                     _lib.stream_ptr(codes.device)), "bh_map_sketch")
        return keys, pos, strand, off

    def _build_index(self):
        dev = self.device
        self._ref = torch.from_numpy(np.concatenate(self._codes)).to(dev)            # the reference codes stay resident
        keys, gpos, strands = [], [], []
        for ci, c in enumerate(self._codes):
            if len(c) < self.k:
                continue
            s = int(self._starts[ci])
            kk, pp, ss, off = self._sketch(self._ref[s:s + len(c)], len(c), np.array([len(c)], np.int32))
            m = int(off[1])
            keys.append(kk[:m])
            gpos.append(pp[:m] + s)
            strands.append(ss[:m])
        keys = torch.cat(keys) if keys else torch.zeros(0, dtype=torch.int64, device=dev)
        # the minimizers arrive in (contig, position) order: a stable sort by key leaves them sorted by (key, contig, position)
        skeys, order = torch.sort(keys, stable=True)
        self._rpos = (torch.cat(gpos)[order] if gpos else torch.zeros(0, dtype=torch.int32, device=dev)).to(torch.int32).contiguous()
        self._rstrand = (torch.cat(strands)[order] if strands else torch.zeros(0, dtype=torch.int8, device=dev)).contiguous()
        self._ukeys, counts = torch.unique_consecutive(skeys, return_counts=True)
        self._ucount = counts.to(torch.int32).contiguous()
        self._ustart = (torch.cumsum(counts, 0) - counts).to(torch.int32).contiguous()
        self._ends = torch.from_numpy(self._starts[1:].copy()).to(dev)
        self.index_keys = skeys                                                      # for inspection and the tests

    def _seed(self, qkeys, qpos, qstrand, qoff, qlen_dev, n, n_min):
        """-> the sorted anchor words of n reads (device int64)"""
        lib = _lib.lib()
        counts = torch.empty(max(n_min, 1), dtype=torch.int32, device=self.device)
        args = (_lib.ptr(qkeys), _lib.ptr(qpos), _lib.ptr(qstrand), _lib.ptr(qoff), _lib.ptr(qlen_dev), n, n_min, _lib.ptr(self._ukeys),
                _lib.ptr(self._ustart), _lib.ptr(self._ucount), int(self._ukeys.numel()), _lib.ptr(self._rpos), _lib.ptr(self._rstrand),
                self.k, self.max_occ, _lib.ptr(counts))
        stream = _lib.stream_ptr(qkeys.device)
        _lib.check(lib.bh_map_seed(*args, None, None, 0, stream), "bh_map_seed")
        ends = torch.cumsum(counts[:n_min].to(torch.int64), 0)
        total = int(ends[-1]) if n_min else 0
        if total == 0:
            return torch.zeros(0, dtype=torch.int64, device=self.device)
        offs = (ends - counts[:n_min]).contiguous()
        anchors = torch.empty(total, dtype=torch.int64, device=self.device)
        _lib.check(lib.bh_map_seed(*args, _lib.ptr(offs), _lib.ptr(anchors), total, stream), "bh_map_seed")
        return torch.sort(anchors).values

    def _chain(self, anchors, n):
        """sorted anchor words -> (offsets [n + 1], f, p, chain, result [n, 4]) on the device"""
        lib = _lib.lib()
        dev = self.device
        total = int(anchors.numel())
        reads = anchors >> (QBITS + RBITS + 1)
        off = torch.searchsorted(reads, torch.arange(n + 1, device=dev, dtype=torch.int64)).to(torch.int32).contiguous()
        gpos = (anchors >> QBITS) & ((1 << RBITS) - 1)
        contig = torch.bucketize(gpos, self._ends, right=True).to(torch.int32).contiguous()
        f = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        p = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        chain = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        result = torch.empty((n, 4), dtype=torch.int32, device=dev)
        _lib.check(lib.bh_map_chain(_lib.ptr(anchors), _lib.ptr(contig), _lib.ptr(off), n, total, self.k, self.max_dist, self.bandwidth,
                                    _lib.ptr(f), _lib.ptr(p), _lib.ptr(chain), _lib.ptr(result), _lib.stream_ptr(anchors.device)),
                   "bh_map_chain")
        return off, contig, f, p, chain, result

    def anchors_of(self, sequences, keep_plane=False):
        """Sketch and seed a batch of at most MAX_READS reads -> (sorted anchor words on the device, list of code arrays); with
        keep_plane the uploaded read plane stays in ``self._plane`` (codes, lengths; both on the device) for ``extend``"""
        n = len(sequences)
        codes = [encode(s) for s in sequences]
        lens = np.array([len(c) for c in codes], np.int32)
        if n and int(lens.max()) > MAX_READ_LEN:
            raise ValueError("map_batch: reads of up to %d bases are supported" % MAX_READ_LEN)
        plane = np.zeros((n, max(1, int(lens.max()) if n else 1)), np.int8)
        for i, c in enumerate(codes):
            plane[i, :len(c)] = c
        dev_plane = torch.from_numpy(plane).to(self.device)
        qkeys, qpos, qstrand, qoff = self._sketch(dev_plane, plane.shape[1], lens)
        self._plane = (dev_plane, torch.from_numpy(lens).to(self.device)) if keep_plane else None
        n_min = int(qoff[n])
        if n_min == 0:
            return torch.zeros(0, dtype=torch.int64, device=self.device), codes
        return self._seed(qkeys, qpos, qstrand, qoff, torch.from_numpy(lens).to(self.device), n, n_min), codes

    def extend(self, plane, lens, ends):
        """The read plane and lengths on the device, numpy int32 ends [n, 6] (read row, strand, side, position on the aligned strand,
        position in the concatenated reference, the contig's limit on that side) -> (numpy result [n, 4]: score, query bases,
        reference bases, runs; a list of the run words per end, in read order). One ``bh_map_extend`` launch."""
        ends = np.ascontiguousarray(ends, np.int32).reshape(-1, 6)
        n = len(ends)
        if n == 0:
            return np.zeros((0, 4), np.int32), []
        cap = 2 * EXT_MAX + EXT_BAND
        dev_ends = torch.from_numpy(ends).to(self.device)
        result = torch.empty((n, 4), dtype=torch.int32, device=self.device)
        runs = torch.empty((n, cap), dtype=torch.int32, device=self.device)
        _lib.check(_lib.lib().bh_map_extend(_lib.ptr(plane), int(plane.shape[1]), _lib.ptr(lens), int(plane.shape[0]), _lib.ptr(self._ref),
                                            int(self._ref.numel()), _lib.ptr(dev_ends), n, _lib.ptr(result), _lib.ptr(runs), cap,
                                            _lib.stream_ptr(plane.device)), "bh_map_extend")
        res = result.cpu().numpy()
        if (res[:, 3] < 0).any():
            raise RuntimeError("bh_map_extend: end %d does not fit its read or its contig" % int(np.argmax(res[:, 3] < 0)))
        width = int(res[:, 3].max())
        words = runs[:, :max(width, 1)].cpu().numpy().view(np.uint32)
        return res, [words[i, :res[i, 3]] for i in range(n)]

    # ---- the batch ---------------------------------------------------------------------------------------------------------------

    def map_batch(self, sequences, extend_ends=None):
        """-> [Mapping or None] in the order given; extend_ends: None = the constructor's value"""
        extend = self.extend_ends if extend_ends is None else bool(extend_ends)
        sequences = [s.upper() for s in sequences]
        out = []
        for lo in range(0, len(sequences), MAX_READS):
            out.extend(self._map_chunk(sequences[lo:lo + MAX_READS], extend))
        return out

    def _tick(self, name, t0):
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        self.timings[name] += t1 - t0
        return t1

    def _map_chunk(self, sequences, extend=False):
        n = len(sequences)
        if n == 0 or not self or not hasattr(self, "_ukeys"):
            return [None] * n
        t = time.perf_counter()
        anchors, codes = self.anchors_of(sequences, keep_plane=extend)
        read_plane, self._plane = self._plane, None
        t = self._tick("sketch_seed", t)
        if anchors.numel() == 0:
            return [None] * n
        off, contig, _f, _p, chain, result = self._chain(anchors, n)
        res = result.cpu().numpy()
        t = self._tick("chain", t)
        off, words, chain, contig = off.cpu().numpy(), anchors.cpu().numpy(), chain.cpu().numpy(), contig.cpu().numpy()
        k = self.k
        plans, seq_rows, ref_rows = [], [], []
        for i in range(n):
            cnt, s1, s2, end = (int(v) for v in res[i])
            if cnt < self.min_cnt or s1 < self.min_score:
                continue
            a0 = int(off[i])
            idx = chain[a0:a0 + cnt][::-1] + a0                                      # the kernel writes the chain last anchor first
            word = words[idx]
            ci = int(contig[idx[0]])
            strand = int((word[0] >> (QBITS + RBITS)) & 1)
            rpos = ((word >> QBITS) & ((1 << RBITS) - 1)) - int(self._starts[ci])
            qpos = word & ((1 << QBITS) - 1)
            q = _COMP[codes[i]][::-1] if strand else codes[i]
            r = self._codes[ci]
            q_st, q_en, r_st, r_en, pieces = span_and_pieces(rpos, qpos, k, q, r)
            mq = min(60, (60 * (s1 - s2)) // s1)
            plans.append((i, ci, strand, q, r, q_st, q_en, r_st, r_en, len(seq_rows), len(pieces), mq // 2 if cnt < 10 else mq))
            for q0, q1, r0, r1 in pieces:
                seq_rows.append(q[q0:q1])
                ref_rows.append(r[r0:r1])
        out = [None] * n
        if not plans:
            self._tick("host", t)
            return out

        def plane(rows):
            m = np.zeros((len(rows), max(1, max(len(x) for x in rows))), np.int8)
            for j, x in enumerate(rows):
                m[j, :len(x)] = np.where(x > 4, 1, x)                                # a non-base is aligned as A
            return m

        sp, rp = plane(seq_rows), plane(ref_rows)
        t = self._tick("host", t)
        if extend:                                                                   # both ends of every mapping in one launch
            ends = np.empty((2 * len(plans), 6), np.int32)
            for x, (i, ci, strand, q, r, q_st, q_en, r_st, r_en, _first, _np, _mq) in enumerate(plans):
                s0 = int(self._starts[ci])
                ends[2 * x] = (i, strand, 0, q_st, s0 + r_st, s0)
                ends[2 * x + 1] = (i, strand, 1, q_en, s0 + r_en, s0 + len(r))
            ext, ext_runs = self.extend(read_plane[0], read_plane[1], ends)
            t = self._tick("extend", t)
        nw = nw_align(sp, rp, cigar=True, device=self.device)
        if (nw.status != 0).any():
            raise RuntimeError("map_batch: a piece did not fit nw_align's workspace budget")
        t = self._tick("base", t)
        for x, (i, ci, strand, q, r, q_st, q_en, r_st, r_en, first, npieces, mapq) in enumerate(plans):
            runs = list(nw.runs[first:first + npieces])
            if extend:
                runs = [ext_runs[2 * x], *runs, ext_runs[2 * x + 1]]
                q_st, r_st = q_st - int(ext[2 * x, 1]), r_st - int(ext[2 * x, 2])
                q_en, r_en = q_en + int(ext[2 * x + 1, 1]), r_en + int(ext[2 * x + 1, 2])
            cigar, cigar_str, nm, md, mlen, blen = finish(np.concatenate(runs), q, r, q_st, r_st)
            if strand:                                                               # on the read as given, like mappy's
                q_st, q_en = len(q) - q_en, len(q) - q_st
            out[i] = Mapping(ctg=self.seq_names[ci], r_st=r_st, r_en=r_en, q_st=q_st, q_en=q_en, strand=-1 if strand else 1, mapq=mapq,
                             cigar=cigar, cigar_str=cigar_str, NM=nm, MD=md, mlen=mlen,
                             blen=blen)
        self._tick("host", t)
        return out


def align_map(aligner, results, batch=256):
    """The (read, result) stream of ``basecall()`` -> the same stream, in the same order, with ``result["mapping"]`` set (a ``Mapping``
    or None); reads are mapped ``batch`` at a time and the last, partial batch is flushed."""
    pending = []

    def flush():
        mappings = aligner.map_batch([res["sequence"] for _, res in pending])
        for (read, res), mapping in zip(pending, mappings):
            yield read, {**res, "mapping": mapping}
        pending.clear()

    for item in results:
        pending.append(item)
        if len(pending) >= batch:
            yield from flush()
    if pending:
        yield from flush()

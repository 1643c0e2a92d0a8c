"""Shared inputs of tests/test_mapper_cpu.py and tests/test_gpu_mapper.py: the planted read set, its expected records from the
restatement (computed once per process), and an independent replay of a record's CIGAR (not taken from tests/mapper_ref.py)."""
import functools
import random
import re

import mapper_ref as M

PLANTED_SEED = 20
CONTIGS = (("ctgA", 30000), ("ctgB", 20000))


def random_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def mutate(rng, seq, rate):
    """substitutions, deletions and insertions, a third of `rate` each"""
    out = []
    for ch in seq:
        x = rng.random()
        if x < rate / 3:
            out.append(rng.choice([c for c in "ACGT" if c != ch]))
        elif x < 2 * rate / 3:
            pass
        elif x < rate:
            out.append(ch)
            out.append(rng.choice("ACGT"))
        else:
            out.append(ch)
    return "".join(out)


@functools.lru_cache(maxsize=None)
def planted(seed=PLANTED_SEED, n_reads=64):
    """-> (contigs [(name, seq)], reads [(sequence, contig index, strand +1 / -1, true start, true end)])"""
    rng = random.Random(seed)
    contigs = [(name, random_seq(rng, n)) for name, n in CONTIGS]
    reads = []
    for i in range(n_reads):
        ci = rng.randrange(len(contigs))
        length = 200 if i == 0 else 3000 if i == 1 else rng.randint(200, 3000)
        start = rng.randrange(0, len(contigs[ci][1]) - length)
        seq = mutate(rng, contigs[ci][1][start:start + length], 0.05)
        strand = 1 if rng.random() < 0.5 else -1
        reads.append((seq if strand == 1 else M.revcomp(seq), ci, strand, start, start + length))
    return contigs, reads


@functools.lru_cache(maxsize=None)
def planted_expected(seed=PLANTED_SEED):
    contigs, reads = planted(seed)
    index = M.Index(contigs)
    return [M.map_read(r[0], index) for r in reads]


def replay(rec, read, contig):
    """One record (a dict or an object with mappy's fields), the read as basecalled and the contig's sequence -> (NM, MD, mlen, blen,
    query bases consumed, reference bases consumed), by walking the CIGAR over the two strings."""
    get = (lambda k: rec[k]) if isinstance(rec, dict) else (lambda k: getattr(rec, k))
    q = read if get("strand") == 1 else M.revcomp(read)
    q_first = get("q_st") if get("strand") == 1 else len(read) - get("q_en")      # q_st / q_en are on the read as basecalled
    qi, ri = q_first, get("r_st")
    nm = mlen = blen = 0
    md, run = "", 0
    for cnt, op in re.findall(r"(\d+)([MID])", get("cigar_str")):
        cnt = int(cnt)
        blen += cnt
        if op == "M":
            for x in range(cnt):
                a, b = q[qi + x], contig[ri + x]
                if a == b and a in "ACGT":
                    run, mlen = run + 1, mlen + 1
                else:
                    md, run, nm = md + "%d%s" % (run, b), 0, nm + 1
            qi, ri = qi + cnt, ri + cnt
        elif op == "I":
            nm, qi = nm + cnt, qi + cnt
        else:
            md, run, nm, ri = md + "%d^%s" % (run, contig[ri:ri + cnt]), 0, nm + cnt, ri + cnt
    return nm, md + "%d" % run, mlen, blen, qi - q_first, ri - get("r_st")


def check_replay(rec, read, contig):
    get = (lambda k: rec[k]) if isinstance(rec, dict) else (lambda k: getattr(rec, k))
    nm, md, mlen, blen, dq, dr = replay(rec, read, contig)
    assert (nm, md, mlen, blen) == (get("NM"), get("MD"), get("mlen"), get("blen"))
    assert dq == get("q_en") - get("q_st") and dr == get("r_en") - get("r_st")
    assert "".join("%d%s" % (c, "MID"[o]) for c, o in get("cigar")) == get("cigar_str")
    assert 0 <= get("q_st") < get("q_en") <= len(read) and 0 <= get("r_st") < get("r_en") <= len(contig)

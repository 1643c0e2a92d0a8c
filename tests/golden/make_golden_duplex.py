"""Writes tests/golden/duplex_cases.json: the outputs of the reference's own duplex functions for seeded inputs.

    python tests/golden/make_golden_duplex.py <path to the reference's bonito/cli/duplex.py>

The reference module is loaded from its file with pysam, mappy, edlib, parasail, tqdm and the bonito.* imports replaced by stub
modules (pysam carries the CIGAR op constants, mappy.revcomp is two lines). Recorded per pair: adj_qscores (both shifts), seq_lens and
trim_while (both ends) on the alignment, compute_consensus, and edlib_adj_align / call_basespace_duplex with edlib.align and
parasail.sg_trace_scan_32 stubbed by the restatements of tests/duplex_ref.py - which pins the reference's glue (splice, trim,
consensus) end to end, given this project's aligner definitions. Needs no GPU; run it where the reference is, commit the JSON."""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import duplex_ref as dr                                                              # noqa: E402

OPS = "MIDNSHP=X"


def load_reference(path):
    def module(name, **attrs):
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
        return mod

    class Traced:
        def __init__(self, text):
            self.cigar = types.SimpleNamespace(decode=text.encode())

    module("pysam", CMATCH=0, CINS=1, CDEL=2, CREF_SKIP=3, CSOFT_CLIP=4, CHARD_CLIP=5, CPAD=6, CEQUAL=7, CDIFF=8)
    module("tqdm", tqdm=lambda it=None, **kw: it)
    module("mappy", revcomp=lambda s: s[::-1].translate(str.maketrans("ACGT", "TGCA")))
    module("edlib", align=lambda q, r, task="path": {"cigar": dr.nw(q, r)[1]})
    module("parasail", dnafull=None,
           sg_trace_scan_32=lambda q, r, o, e, matrix: Traced(dr.sg(q, r, 5, -4, o, e)[1]))
    module("bonito")
    module("bonito.io", DuplexWriter=None, biofmt=None)
    module("bonito.aligner", align_map=None, Aligner=None)
    module("bonito.multiprocessing", ProcessMap=None)
    module("bonito.util", tqdm_environ=None)
    spec = importlib.util.spec_from_file_location("reference_duplex", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def number(v):
    """float32 -> an int where it is whole, otherwise the shortest decimal that reads back to the same float32"""
    return int(v) if float(v).is_integer() else float(np.format_float_positional(np.float32(v), unique=True))


def text(cigartuples):
    return "".join("%d%s" % (n, OPS[op]) for op, n in cigartuples)


def rand_seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, size=n))


def with_runs(rng, n):
    out = []
    while len(out) < n:
        out.extend("ACGT"[int(rng.integers(0, 4))] * int(rng.choice([1, 1, 1, 2, 3, 5, 9])))
    return "".join(out[:n])


def mutate(rng, s, rate):
    out = []
    for ch in s:
        u = rng.random()
        if u < rate / 3:
            out.append("ACGT"[("ACGT".index(ch) + int(rng.integers(1, 4))) % 4])
        elif u < 2 * rate / 3:
            out.extend([ch, "ACGT"[int(rng.integers(0, 4))]])
        elif u >= rate:
            out.append(ch)
    return "".join(out)


def cases():
    rng = np.random.default_rng(20)
    rc = dr.revcomp
    out = []

    def add(name, temp, comp_fwd, quals="random"):
        """comp_fwd: the complement strand as it aligns to the template (the stored complement call is its reverse complement)"""
        comp = rc(comp_fwd)
        if quals == "flat":
            tq, cq = [20] * len(temp), [20] * len(comp)
        else:
            tq, cq = rng.integers(2, 51, size=len(temp)).tolist(), rng.integers(2, 51, size=len(comp)).tolist()
        out.append(dict(name=name, temp_seq=temp, temp_qstring=bytes(v + 33 for v in tq).decode(), comp_seq=comp,
                        comp_qstring=bytes(v + 33 for v in cq).decode()))

    for n in (40, 150, 300, 600):
        core = rand_seq(rng, n)
        for k in range(2):
            oh = [int(v) for v in rng.integers(0, 61, size=4)]
            oh[int(rng.integers(0, 4))] = 0
            temp = rand_seq(rng, oh[0]) + core + rand_seq(rng, oh[1])
            comp = rand_seq(rng, oh[2]) + mutate(rng, core, 0.05) + rand_seq(rng, oh[3])
            add("random_%d_%d" % (n, k), temp, comp)
    core = with_runs(rng, 300)
    add("homopolymers", rand_seq(rng, 30) + core, mutate(rng, core, 0.05) + rand_seq(rng, 25))
    add("homopolymers_flat", core, mutate(rng, core, 0.05), quals="flat")
    add("no_long_match", rand_seq(rng, 60), rand_seq(rng, 70))
    add("short_identical", core[:8], core[:8])
    add("identical", core[:120], core[:120])
    mid = core[:60] + mutate(rng, core[60:200], 0.08) + core[200:260]
    add("long_match_at_both_ends", core[:260], mid)
    add("ties", core[:200], mutate(rng, core[:200], 0.05), quals="flat")
    add("tail_overhang_only", core[:180], mutate(rng, core[:180], 0.05) + rand_seq(rng, 40))
    add("head_overhang_only", rand_seq(rng, 45) + core[:180], mutate(rng, core[:180], 0.05))
    return out


def main():
    ref = load_reference(sys.argv[1])
    records = []
    for c in cases():
        tq = np.frombuffer(c["temp_qstring"].encode(), np.uint8) - np.uint8(33)           # Phred scores, as pysam hands them over
        cq = np.frombuffer(c["comp_qstring"].encode(), np.uint8) - np.uint8(33)
        adj_t = ref.adj_qscores(tq, c["temp_seq"], qshift=1)
        adj_c = ref.adj_qscores(cq, c["comp_seq"], qshift=-1)
        comp_rc = dr.revcomp(c["comp_seq"])
        cigar = ref.edlib_adj_align(c["temp_seq"], comp_rc)
        q_len, r_len = ref.seq_lens(cigar)
        head, ts, cs = ref.trim_while(cigar)
        both, te, ce = ref.trim_while(head, from_end=True)
        seq, qstring = ref.call_basespace_duplex(c["temp_seq"], tq.tobytes(), c["comp_seq"], cq.tobytes())
        rec = dict(c, adj_temp=[number(v) for v in adj_t], adj_comp=[number(v) for v in adj_c], nw_cigar=dr.nw(c["temp_seq"], comp_rc)[1],
                   cigar=text(cigar), seq_lens=[int(q_len), int(r_len)], trim_start=[text(head), int(ts), int(cs)],
                   trim_end=[text(both), int(te), int(ce)], sequence=seq, qstring=qstring)
        assert adj_t.dtype == np.float32 and (q_len, r_len) == (len(c["temp_seq"]), len(comp_rc))
        if len(both):
            t, r = c["temp_seq"], comp_rc
            rec["consensus"] = list(ref.compute_consensus(both, t[ts:len(t) - te], adj_t[ts:len(t) - te], r[cs:len(r) - ce],
                                                          adj_c[::-1][cs:len(r) - ce]))
            assert rec["consensus"] == [seq, qstring]
        else:
            assert (seq, qstring) == ("", "")
        records.append(rec)
    with open(os.path.join(HERE, "duplex_cases.json"), "w") as fh:
        json.dump(dict(num_match=11, cases=records), fh, separators=(",", ":"))
        fh.write("\n")
    for r in records:
        print("%-26s %4d %4d  %-40.40s -> %d bases" % (r["name"], len(r["temp_seq"]), len(r["comp_seq"]), r["cigar"], len(r["sequence"])))


if __name__ == "__main__":
    main()

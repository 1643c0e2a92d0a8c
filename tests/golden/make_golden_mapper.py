"""Writes tests/golden/mapper_sam_cases.json: the outputs of the reference's own sam_record and summary_row for hand-made mapping
records (both strands, with and without soft-clips at either end, an unmapped read).

    python tests/golden/make_golden_mapper.py <path to the reference's bonito/io.py>

The reference module is loaded from its file with pandas, mappy, pysam and the bonito.* imports replaced by stub modules
(mappy.revcomp is two lines). Only the JSON of inputs and recorded strings is committed. Needs no GPU; run it where the reference
is."""
import importlib.util
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))

READ = dict(filename="batch_0.pod5", read_id="7d5a3c1e-read", run_id="run_a1", channel=12, mux=3, start=101.25, duration=2.5,
            template_start=101.5, template_duration=2.25)
SEQ = "ACGTTGCAAGGCTTAACCGGTATCGATTGCAGT"                                            # 33 bases


def mapping(strand, q_st, q_en, cigar, nm, md, mlen, blen, ctg="chr1", r_st=1000, mapq=60):
    r_len = sum(n for n, op in cigar if op != 1)
    return dict(ctg=ctg, r_st=r_st, r_en=r_st + r_len, q_st=q_st, q_en=q_en, strand=strand, mapq=mapq, cigar=cigar,
                cigar_str="".join("%d%s" % (n, "MID"[op]) for n, op in cigar), NM=nm, MD=md, mlen=mlen, blen=blen)


CASES = [
    ("plus_whole", mapping(+1, 0, 33, [[33, 0]], 0, "33", 33, 33)),
    ("minus_whole", mapping(-1, 0, 33, [[33, 0]], 1, "10A22", 32, 33)),
    ("plus_clip_start", mapping(+1, 5, 33, [[28, 0]], 2, "3C10T13", 26, 28)),
    ("plus_clip_end", mapping(+1, 0, 29, [[29, 0]], 0, "29", 29, 29, mapq=3)),
    ("plus_clip_both", mapping(+1, 4, 30, [[10, 0], [2, 1], [14, 0]], 2, "24", 24, 26, ctg="ctgB", r_st=0)),
    ("minus_clip_start", mapping(-1, 6, 33, [[12, 0], [3, 2], [15, 0]], 4, "12^ACG7G7", 26, 30)),
    ("minus_clip_end", mapping(-1, 0, 25, [[25, 0]], 0, "25", 25, 25, mapq=0)),
    ("minus_clip_both", mapping(-1, 2, 31, [[9, 0], [1, 1], [8, 0], [2, 2], [11, 0]], 5, "5T3A7^TT11", 26, 31)),
    ("plus_indels", mapping(+1, 0, 33, [[5, 0], [4, 1], [10, 0], [6, 2], [14, 0]], 11, "15^GATTAC0A13", 28, 39, mapq=30)),
    ("minus_one_base_clips", mapping(-1, 1, 32, [[31, 0]], 3, "0A29T0", 28, 31, mapq=17)),
    ("plus_tags", mapping(+1, 3, 33, [[30, 0]], 0, "30", 30, 30)),
    ("unmapped", None),
]
TAGS = {"plus_tags": ["RG:Z:run_a1", "qs:f:12.50", "ns:i:4000"], "unmapped": ["RG:Z:run_a1"]}


def load_reference(path):
    def module(name, **attrs):
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
        return mod

    module("pandas")
    module("mappy", __version__="stub", revcomp=lambda s: s[::-1].translate(str.maketrans("ACGT", "TGCA")))
    module("pysam", AlignmentFile=None, AlignmentHeader=None, AlignedSegment=None)
    module("bonito", __version__="stub")
    module("bonito.util", mean_qscore_from_qstring=None)
    spec = importlib.util.spec_from_file_location("reference_io", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_reference(sys.argv[1])
    read = types.SimpleNamespace(**READ)
    qstring = "".join(chr(33 + 5 + (i * 7) % 30) for i in range(len(SEQ)))
    out = dict(read=READ, sequence=SEQ, qstring=qstring, qscore=12.5, field_names=ref.summary_field_names, cases=[])
    for name, m in CASES:
        obj = None
        if m is not None:
            obj = types.SimpleNamespace(**m)
            obj.cigar = [tuple(c) for c in m["cigar"]]
        row = ref.summary_row(read, len(SEQ), 12.5, alignment=obj)
        out["cases"].append(dict(name=name, mapping=m, tags=TAGS.get(name),
                                 sam=ref.sam_record(READ["read_id"], SEQ, qstring, obj, tags=TAGS.get(name)),
                                 summary=[row[k] for k in ref.summary_field_names]))
    with open(os.path.join(HERE, "mapper_sam_cases.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()

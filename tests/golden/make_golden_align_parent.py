"""Writes tests/golden/align_parent.json: what the pairwise aligners' host side computed BEFORE their shared parts were folded into
csrc/pair_align.h and one slicer in bonito_amd/align.py.

    git checkout 283cf20 && python build.py && python tests/golden/make_golden_align_parent.py 283cf20

It runs at that parent commit only (it calls the parent's ``_slices`` and ``_nw_slices``, which no longer exist) and needs no GPU:
the workspace functions are host code. Recorded: ``bh_sw_workspace`` and ``bh_nw_workspace`` over a sweep of their arguments, and
the slices (index lists, maxima, unfit pairs or the ValueError's text) of seeded length pairs at three budgets, and at a fourth that
the first 40 pairs of the order fill to the byte (none of the three round budgets is met exactly, so they alone would not tell
``>`` from ``>=`` in the slicer).
tests/test_align_cpu.py asserts that the present library and slicer reproduce every row."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

COUNTS = (1, 2, 3, 512)
SW_LENGTHS = (0, 1, 511, 512, 513, 4096)
NW_LENGTHS = (0, 1, 511, 512, 513, 1100, 65536)
NW_BANDS = (1, 129, 1025, 131073)
BUDGETS = (1 << 20, 8 << 20, 1 << 30)
NW_K = (64, 512)


def lengths():
    """200 (seq, ref) length pairs: 190 drawn as tests/test_gpu_duplex.py draws its mixed batch (the query a few percent off its
    reference, some empty, some unrelated), then ten between 2000 and 4096."""
    rng = np.random.default_rng(14)
    seq, ref = [], []
    for k in range(190):
        n = int(rng.choice([0, 1, 5, 40, 200, 511, 513, 700, 1300]) + rng.integers(0, 30)) if k % 16 else 0
        s = 0 if k % 37 == 0 else max(0, n + int(rng.integers(-(n // 20) - 1, n // 20 + 2)))
        if k % 11 == 0:
            s = int(rng.integers(0, 600))
        seq.append(s); ref.append(n)
    for _ in range(10):
        seq.append(int(rng.integers(2000, 4097))); ref.append(int(rng.integers(2000, 4097)))
    return np.array(seq, np.int32), np.array(ref, np.int32)


def sw_order(sl, rl):
    return np.argsort(((sl.astype(np.int64) + 511) // 512) * (rl.astype(np.int64) + 63), kind="stable")


def nw_order(sl, rl, k):
    size = ((sl.astype(np.int64) + 511) // 512) * np.minimum(rl.astype(np.int64), 511 + np.abs(rl - sl) + 2 * k + 1)
    return np.argsort(size, kind="stable")


def main():
    from bonito_amd import _lib
    from bonito_amd.align import _nw_slices, _slices
    lib = _lib.lib()
    sw_ws = [[n, s, r, lib.bh_sw_workspace(n, s, r)] for n in COUNTS for s in SW_LENGTHS for r in SW_LENGTHS]
    nw_ws = [[n, s, r, b, lib.bh_nw_workspace(n, s, r, b)] for n in COUNTS for s in NW_LENGTHS for r in NW_LENGTHS for b in NW_BANDS]
    sl, rl = lengths()
    short = np.flatnonzero((sl <= 1000) & (rl <= 1000))                   # the local aligner at the small budgets: every pair fits
    sw, nw = [], []
    head = sw_order(sl, rl)[:40]
    for budget in BUDGETS + (lib.bh_sw_workspace(40, int(sl[head].max()), int(rl[head].max())),):
        for which, pick in (("all", np.arange(len(sl))), ("short", short)):
            row = dict(budget=budget, pairs=which)
            try:
                got = _slices(pick[sw_order(sl[pick], rl[pick])], sl, rl, budget, lib)
                row["slices"] = [[idx.tolist(), int(ms), int(mr)] for idx, ms, mr in got]
            except ValueError as e:
                row["raises"] = str(e)
            sw.append(row)
    for k in NW_K:
        head = nw_order(sl, rl, k)[:40]
        exact = lib.bh_nw_workspace(40, int(sl[head].max()), int(rl[head].max()), int(np.abs(rl[head] - sl[head]).max()) + 2 * k + 1)
        for budget in BUDGETS + (exact,):
            got, unfit = _nw_slices(nw_order(sl, rl, k), sl, rl, k, budget, lib)
            nw.append(dict(budget=budget, k=k, slices=[[idx.tolist(), int(ms), int(mr), int(mb)] for idx, ms, mr, mb in got],
                           unfit=[int(i) for i in unfit]))
    with open(os.path.join(HERE, "align_parent.json"), "w") as fh:
        json.dump(dict(parent=sys.argv[1], seq_len=sl.tolist(), ref_len=rl.tolist(), sw_workspace=sw_ws, nw_workspace=nw_ws,
                       sw_slices=sw, nw_slices=nw), fh, separators=(",", ":"))
        fh.write("\n")
    print("%d + %d workspace rows; sw: %s; nw: %s" % (len(sw_ws), len(nw_ws),
          [len(r.get("slices", [])) or "raises" for r in sw], [(len(r["slices"]), len(r["unfit"])) for r in nw]))


if __name__ == "__main__":
    main()

"""The recurrent kernels' launch side (the instance table, lstm_launch_plan and q8_launch_plan of csrc/lstm.hip / lstm_q8.hip, read
through the test hook bh_lstm_launch_plan) against tests/golden/lstm_plan_parent.json: what the host code of the commit BEFORE the table
existed - seven launchers, their width checks and ladders - accepted, launched and armed for the same calls, recorded from that commit
(profiles/lstm_launch_parent_vs_branch.txt says how). No GPU: the hook touches none.

The sweep: every fp16 family x H = 16, 32, ..., 1088 (every multiple of 16, so that the widths between two instances are in it) x CUs
{8, 64, 256}; where the family serves H, n_rings in {1, 3, per, per + 1} with per = the rings one launch held on the parent (the
ring-in-a-workgroup family, which has no such limit: {1, 3, 129}); the wide family also with the hand-off through the output tensor
(flags bit 1); (wgx2, 384) and (wide, 1024) also with "lstm_tune" bit 2. The 8-bit family: H = 16, ..., 528 x variant {0, 1, 2} x CUs
{8, 256} x the same n_rings. A row is key + `refused` + the hook's record; of a refused launch the record ends behind
rings_per_launch."""
import ctypes as C
import json
import os

import pytest

from conftest import GOLDEN
from bonito_amd import _lib
from test_abi import _family_call

KEY = ["family", "H", "flags", "cus", "n_rings"]
FIELDS = ["serves", "ring_chunks", "wgs_per_group", "rings_per_slot", "wgs_per_cu", "unlimited", "rings_per_launch",
          "grid", "block", "lds_bytes", "lds_raised", "xcc_bytes", "arm_bytes", "ex_ring_stride", "key_nks", "key_mt", "key_flags"]
N_HEAD = FIELDS.index("rings_per_launch") + 1           # what a refused launch still reports
TUNE_STATS = 4 << 8
Q8 = _lib.LSTM_FAMILIES["q8"]
WGX2, WIDE = _lib.LSTM_FAMILIES["wgx2"], _lib.LSTM_FAMILIES["wide"]


def sweep_cases():
    """(family, H, flags, cus), in the golden's order."""
    cases = []
    for family in range(Q8):
        for H in range(16, 1089, 16):
            for cus in (8, 64, 256):
                flags = [0] + ([2] if family == WIDE else []) + ([TUNE_STATS] if (family, H) in ((WGX2, 384), (WIDE, 1024)) else [])
                cases += [(family, H, f, cus) for f in flags]
    cases += [(Q8, H, variant, cus) for H in range(16, 529, 16) for variant in (0, 1, 2) for cus in (8, 256)]
    return cases


def read_plan(family, H, flags, cus, n_rings):
    out = (C.c_int32 * len(FIELDS))()
    rc = _lib.lib().bh_lstm_launch_plan(family, H, flags, n_rings, cus, out, len(FIELDS))
    return rc, list(out)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "lstm_plan_parent.json")) as f:
        g = json.load(f)
    assert g["key"] == KEY and g["fields"] == FIELDS
    return g


def test_header_record_length():
    text = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "bonito_hip.h")).read()
    assert "enum { BH_LSTM_PLAN_RECORD = %d };" % len(FIELDS) in text


def test_golden_covers_the_sweep(golden):
    by_case = {}
    for row in golden["rows"]:
        by_case.setdefault(tuple(row[:4]), []).append(row)
    assert list(by_case) == sweep_cases()
    for case, rows in by_case.items():
        serves, unlimited, per = (rows[0][6 + FIELDS.index(f)] for f in ("serves", "unlimited", "rings_per_launch"))
        rings = [r[4] for r in rows]
        assert rings == ([1] if not serves else [1, 3, 129] if unlimited else sorted({1, 3, per, per + 1})), case
        for r in rows:       # the parent refused exactly: a width without an instance, no ring, more rings than a launch holds
            assert r[5] == int(not serves or not (unlimited or 1 <= r[4] <= per)), r[:6]


def test_plan_equals_what_the_parent_launched(golden):
    for row in golden["rows"]:
        (family, H, flags, cus, n_rings), refused, want = row[:5], row[5], row[6:]
        rc, got = read_plan(family, H, flags, cus, n_rings)
        where = dict(zip(KEY, row[:5]))
        assert (rc != 0) == bool(refused), (where, _lib.last_error())
        n = N_HEAD if refused else len(FIELDS)
        assert got[:n] == want[:n], (where, [(f, g, w) for f, g, w in zip(FIELDS, got[:n], want) if g != w])


def test_every_instance_launches_and_every_other_width_is_refused(golden):
    """serves <=> one ring is launchable on 256 CUs; a (family, H) that does not serve is refused by the hook AND by the argument
    check of bh_lstm_layer_family (in front of any device call: the pointers are never read)."""
    seen = set()
    for family, H, flags, cus in sweep_cases():
        if cus != 256 or (family, H) in seen or family == Q8:
            continue
        seen.add((family, H))
        rc, got = read_plan(family, H, 0, 256, 1)
        assert (rc == 0) == bool(got[0]), (family, H)
        if rc != 0:
            assert "has no instance" in _lib.last_error(), (family, H)
            rc_abi, msg = _family_call(family, H)
            assert rc_abi != 0 and "has no instance for hidden size %d" % H in msg, (family, H, msg)
    assert len(seen) == 7 * 68


def test_plan_hook_refuses_bad_arguments():
    out = (C.c_int32 * len(FIELDS))()
    handle = _lib.lib()
    assert handle.bh_lstm_launch_plan(0, 96, 0, 1, 256, out, len(FIELDS) - 1) != 0 and "%d" % len(FIELDS) in _lib.last_error()
    assert handle.bh_lstm_launch_plan(0, 96, 0, 1, 256, None, len(FIELDS)) != 0
    assert handle.bh_lstm_launch_plan(8, 96, 0, 1, 256, out, len(FIELDS)) != 0
    assert handle.bh_lstm_launch_plan(-1, 96, 0, 1, 256, out, len(FIELDS)) != 0
    assert handle.bh_lstm_launch_plan(0, 96, 0, 1, 0, out, len(FIELDS)) != 0
    assert handle.bh_lstm_launch_plan(3, 96, 2, 1, 256, out, len(FIELDS)) != 0 and "exchange buffer" in _lib.last_error()

"""The decode stage's launch plan and workspace layout (beam_plan / decode_workspace in csrc/beam.hip, read through the test hook
bh_beam_search_plan) against tests/golden/beam_plan_parent.json: what the host code of the commit BEFORE the plan existed launched and
carved for the same calls, recorded from that commit (profiles/beam_plan_parent_vs_branch.txt says how). No GPU: the hook touches none.

The sweep of the issue is state_len 1-5 x CUs {8, 256} x N {1, 5 CUs, 5 CUs + 1, 6 CUs, 6 CUs + 1, 2048} x T {1, 7, 1667} x beam_fuse
{-1, 0, 1} x beam_cpw {0..4} x beam_fork {-1, 0, 1} x beam_select {0, 1} x debug {0, 1}: 32400 calls. Pruned, each for a reason that can
be read off the host code on BOTH sides of the comparison:
  * T reaches nothing but the byte sizes of the workspace regions, and those read no option, no CU count and no debug flag: the layout
    is swept over (state_len, N, T) alone, the plan at one T.
  * beam_select reaches only the selection scale of BeamArgs, which nothing else reaches: both values, once per state_len.
  * beam_fork reaches only the stream of the stand-alone forward scan; beam_cpw and debug reach only the beam kernel's instance: fork
    0 / 1 are swept at beam_cpw 0 without debug, beam_cpw and debug at beam_fork -1 (beam_fuse, which both depend on, stays crossed
    with each).
  * The CU count is read only by the automatic beam_cpw at state_len 4: the other state lengths run at 8 CUs, where beam_cpw is swept
    over {0, 2} (it is ignored there, 2 shows it)."""
import ctypes as C
import json
import os

import pytest

from conftest import GOLDEN
from bonito_amd import _lib

PLAN_KEY = ["state_len", "cus", "N", "beam_fuse", "beam_cpw", "beam_fork", "beam_select", "debug"]
PLAN_FIELDS = ["bwd_state_len", "bwd_grid", "bwd_block", "bwd_lds",
               "fwd_present", "fwd_state_len", "fwd_grid", "fwd_block", "fwd_lds", "fwd_on_helper_stream",
               "beam_state_len", "beam_cpw", "beam_dbg", "beam_fuse", "beam_grid", "beam_block", "beam_lds",
               "select_radix", "decode_nt"]
WS_KEY = ["state_len", "N", "T"]
WS_FIELDS = ["beta", "Bcum", "logZ", "P", "bp", "final_slot", "debug_counters", "posterior_viterbi_bp", "beam_total",
             "posterior_viterbi_total"]
N_RECORD = len(PLAN_FIELDS) + 2 * len(WS_FIELDS)        # bh_beam_search_plan: the layout as (low, high) halves
T_PLAN = 7
DEFAULTS = {"beam_fuse": -1, "beam_cpw": 0, "beam_fork": -1, "beam_select": 0}


def _batch_sizes(cus):
    return [1, 5 * cus, 5 * cus + 1, 6 * cus, 6 * cus + 1, 2048]


def plan_sweep():
    """Rows of PLAN_KEY."""
    rows = []
    for sl in (1, 2, 3, 4, 5):
        for cus in ((8, 256) if sl == 4 else (8,)):
            for n in _batch_sizes(cus):
                for fuse in (-1, 0, 1):
                    for cpw in ((0, 1, 2, 3, 4) if sl == 4 else (0, 2)):
                        for debug in (0, 1):
                            rows.append((sl, cus, n, fuse, cpw, -1, 0, debug))
                    for fork in (0, 1):
                        rows.append((sl, cus, n, fuse, 0, fork, 0, 0))
        rows.append((sl, 8, 41, -1, 0, -1, 1, 0))
    return rows


def workspace_sweep():
    """Rows of WS_KEY."""
    sizes = sorted(set(_batch_sizes(8) + _batch_sizes(256)))
    return [(sl, n, t) for sl in (1, 2, 3, 4, 5) for n in sizes for t in (1, 7, 1667)]


def read_plan(handle, n, t, sl, cus, debug):
    """One call of the hook -> (plan fields, layout fields)."""
    out = (C.c_int32 * N_RECORD)()
    _lib.check(handle.bh_beam_search_plan(n, t, sl, cus, debug, out, N_RECORD), "bh_beam_search_plan")
    rec = list(out)
    k = len(PLAN_FIELDS)
    layout = [(rec[k + 2 * i] & 0xffffffff) | (rec[k + 2 * i + 1] << 32) for i in range(len(WS_FIELDS))]
    return rec[:k], layout


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "beam_plan_parent.json")) as f:
        g = json.load(f)
    assert g["plan_key"] == PLAN_KEY and g["plan_fields"] == PLAN_FIELDS
    assert g["workspace_key"] == WS_KEY and g["workspace_fields"] == WS_FIELDS
    return g


@pytest.fixture()
def options():
    handle = _lib.lib()

    def set_options(**kw):
        for name, value in kw.items():
            _lib.check(handle.bh_set_option(name.encode(), value), "bh_set_option")
    try:
        yield set_options
    finally:
        set_options(**DEFAULTS)


def test_plan_equals_what_the_parent_launched(golden, options):
    handle = _lib.lib()
    sweep = plan_sweep()
    assert [tuple(r[:len(PLAN_KEY)]) for r in golden["plan_rows"]] == sweep
    for row in golden["plan_rows"]:
        key, want = row[:len(PLAN_KEY)], row[len(PLAN_KEY):]
        sl, cus, n, fuse, cpw, fork, select, debug = key
        options(beam_fuse=fuse, beam_cpw=cpw, beam_fork=fork, beam_select=select)
        got, _ = read_plan(handle, n, T_PLAN, sl, cus, debug)
        assert got == want, dict(zip(PLAN_KEY, key), differs=[(f, g, w) for f, g, w in zip(PLAN_FIELDS, got, want) if g != w])


def test_workspace_layout_equals_the_parents(golden):
    handle = _lib.lib()
    sweep = workspace_sweep()
    assert [tuple(r[:len(WS_KEY)]) for r in golden["workspace_rows"]] == sweep
    for row in golden["workspace_rows"]:
        (sl, n, t), want = row[:len(WS_KEY)], row[len(WS_KEY):]
        _, got = read_plan(handle, n, t, sl, 8, 0)
        assert got == want, (sl, n, t, [(f, g, w) for f, g, w in zip(WS_FIELDS, got, want) if g != w])
        # callers allocate by the two exports
        assert handle.bh_beam_search_workspace(n, t, sl) == want[WS_FIELDS.index("beam_total")]
        assert handle.bh_crf_posterior_viterbi_workspace(n, t, sl) == want[WS_FIELDS.index("posterior_viterbi_total")]
        # every region is 256-byte aligned, in order, and the last one ends inside the total
        offs = got[:7]
        assert all(o % 256 == 0 for o in offs) and offs == sorted(offs) and offs[0] == 0
        assert offs[6] + n * 8 * 8 <= got[8] == got[7] and got[7] + n * t * 4 ** sl <= got[9]


def test_plan_hook_refuses_bad_arguments():
    handle = _lib.lib()
    out = (C.c_int32 * N_RECORD)()
    assert handle.bh_beam_search_plan(4, 7, 0, 8, 0, out, N_RECORD) != 0 and "state_len" in _lib.last_error()
    assert handle.bh_beam_search_plan(0, 7, 3, 8, 0, out, N_RECORD) != 0
    assert handle.bh_beam_search_plan(4, 7, 3, 8, 0, out, N_RECORD - 1) != 0 and "%d" % N_RECORD in _lib.last_error()
    assert handle.bh_beam_search_plan(4, 7, 3, 8, 0, None, N_RECORD) != 0

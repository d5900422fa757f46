"""not-gpu: which form acgpu_count_patterns takes (plan_count, aho-corasick_amd/csrc/host/engine_plan.hpp) as a table: state
visits on the LDS walk, or the records of the overlapping search.  Both return identical counts; the plan decides cost."""
import ctypes as C

import pytest

import aho_corasick_amd as ac

VISITS, RECORDS = 1, 0


@pytest.mark.parametrize("facts,want", [
    (dict(), VISITS),                         # LDS image, no empty pattern, automatic engine choice
    (dict(want=2), VISITS),                   # the LDS walk requested
    (dict(lw=0), RECORDS),                    # no LDS image: a large set, or a split set (asked without one)
    (dict(lw=0, want=2), RECORDS),            # ... the overlapping search then refuses the engine
    (dict(min_len=0), RECORDS),               # an empty pattern: every state is a match state
    (dict(min_len=0, want=2), RECORDS),
    (dict(want=1), RECORDS),                  # a forced transition walk
    (dict(want=3), RECORDS),                  # a forced prefix filter
    (dict(count_hist=0), RECORDS),            # the variant
    (dict(count_hist=0, want=2), RECORDS),
    (dict(count_hist=2), VISITS),             # (2: state visits without the hot-bin shortcut)
])
def test_count_plan_table(facts, want):
    f = dict(dict(lw=1, min_len=3, want=0, count_hist=1), **facts)
    out = (C.c_uint32 * 1)()
    arr = (C.c_uint64 * 4)(f["lw"], f["min_len"], f["want"], f["count_hist"])
    assert ac.load_test_hooks().acgpu_test_count_plan(None, arr, out) == 0
    assert out[0] == want, facts

"""not-gpu: the sizing rules of the overlapping search (aho-corasick_amd/csrc/host/ov_sizes.hpp -- the functions both of its
orchestrations, capi_overlap.cpp and capi_enqueue.cpp, call) as a table: event-list capacity, the order pass's bounds next to
the capacity the scan is launched with (a call that has read the counts back sizes the pass by the counts themselves), halo, chunk grids, eligibility of the LDS walk's event form.  The expected values are
written out by hand from the rules, not computed by the library."""
import ctypes as C

import pytest

import aho_corasick_amd as ac

CAPACITY, GUESSED, HINTED, HALO, GRID, FILL_GRID, LW_EVENTS = range(7)
MAX_EV = 12 << 20          # kSortMaxEvents = 12 582 912
ALL_PAIRS = 16384          # kEvAllPairs
GIB = 1 << 30              # its event list is capped: (1 << 30) / 64 = 16 777 216 > MAX_EV


def rule(which, a=0, b=0, c=0):
    L = ac.load_test_hooks()
    out = (C.c_uint64 * 3)()
    assert L.acgpu_test_ov_sizes(which, a, b, c, out) == 0
    return tuple(out)


@pytest.mark.parametrize("span,want", [
    (0, 65536),                       # never fewer than 2^16 events
    ((64 << 16) - 1, 65536),          # span / 64 = 65 535
    (64 << 16, 65536),
    ((64 << 16) + 63, 65536),
    ((64 << 16) + 64, 65537),         # ... one event per 64 haystack bytes from here on
    (1 << 28, 4194304),
    (64 * MAX_EV - 1, 12582911),      # 768 MiB - 1
    (64 * MAX_EV, 12582912),          # capped at kSortMaxEvents
    (1 << 40, 12582912),
])
def test_event_list_capacity(span, want):
    assert rule(CAPACITY, span)[0] == want


@pytest.mark.parametrize("which,args,want", [
    # a guessed stream: never within the all-pairs rank's range, never beyond the event list; records = the caller's room
    (GUESSED, (GIB, 100, 200), (12582912, 16385, 200)),            # guess below kEvAllPairs
    (GUESSED, (GIB, ALL_PAIRS, 65536), (12582912, 16385, 65536)),
    (GUESSED, (GIB, 90000, 131072), (12582912, 90000, 131072)),
    (GUESSED, (0, 1000000, 2000000), (65536, 65536, 2000000)),     # guess above cap_ev
    # only the density hint: the whole event list, and min(cap, 2^26, 4 * cap_ev) records
    (HINTED, (0, 0, 1000), (65536, 65536, 1000)),                  # cap below 4 * cap_ev = 262 144
    (HINTED, (0, 0, 262144), (65536, 65536, 262144)),
    (HINTED, (0, 0, 300000), (65536, 65536, 262144)),              # cap above it
    (HINTED, (GIB, 0, 50331647), (12582912, 12582912, 50331647)),  # 4 * kSortMaxEvents = 50 331 648 ...
    (HINTED, (GIB, 0, 60000000), (12582912, 12582912, 50331648)),  # ... which lies below 2^26 = 67 108 864
    (HINTED, (GIB, 0, (1 << 26) - 1), (12582912, 12582912, 50331648)),
    (HINTED, (GIB, 0, (1 << 26) + 5), (12582912, 12582912, 50331648)),
])
def test_order_bounds_come_with_the_scan_capacity(which, args, want):
    assert rule(which, *args) == want


@pytest.mark.parametrize("max_pattern_len,halo,ok", [
    (0, 0, 1), (1, 0, 1), (2, 1, 1), (65536, 65535, 1),
    (0xFFFFFF01, 0xFFFFFF00, 1),
    (0xFFFFFF01 + 1, 0xFFFFFF01, 0),      # one past the limit
])
def test_halo_and_its_limit(max_pattern_len, halo, ok):
    assert rule(HALO, max_pattern_len)[:2] == (halo, ok)


@pytest.mark.parametrize("lo,hi,chunk,grid0,n", [
    (0, 0, 2048, 0, 1),                   # an empty window still has one chunk
    (1000, 5000, 512, 512, 9),            # emit_lo not on the grid: (5000 - 512 + 511) / 512 = 9
    (1000, 1000, 512, 512, 1),            # emit_hi == emit_lo, off the grid
    (1024, 1024, 512, 1024, 1),           # ... and on it
    (1024, 2048, 512, 1024, 2),
    (1024, 2049, 512, 1024, 3),
])
def test_chunk_grid(lo, hi, chunk, grid0, n):
    assert rule(GRID, lo, hi, chunk)[:2] == (grid0, n)


def test_the_chunk_fill_takes_four_lane_chunks_at_a_time():
    assert rule(FILL_GRID, 512, 9)[:2] == (2048, 3)
    assert rule(FILL_GRID, 512, 8)[:2] == (2048, 2)
    assert rule(FILL_GRID, 256, 1)[:2] == (1024, 1)


def test_event_form_of_the_lds_walk_is_for_spans_below_15_gib():
    assert rule(LW_EVENTS, 3, 1, (15 << 30) - 1)[0] == 1
    assert rule(LW_EVENTS, 3, 1, 15 << 30)[0] == 0
    assert rule(LW_EVENTS, 3, 1, 0)[0] == 1
    assert rule(LW_EVENTS, 3, 0, 1 << 20)[0] == 0      # an empty pattern
    assert rule(LW_EVENTS, 1, 4, 1 << 20)[0] == 0      # variant lw_events = 0
    assert rule(LW_EVENTS, 2, 4, 1 << 20)[0] == 0      # another engine runs first

"""-m gpu: the long segments of the batched find on the device (device/batch_long.hip): record s against the oracle's find
on the span (off[s], off[s+1]) with variant batch_lane_max = 2 T, so that "long" is small -- every match kind, anchored and
earliest modes, every scout stepper, plants on every edge of the window / lane-chunk grid, one segment across the grid, and
the single-span calls that remain.  Integers: equality."""
import functools

import numpy as np
import pytest
import torch

import aho_corasick_amd as ac
from aho_corasick_amd import _lib
from gpu_util import build_pair
from test_gpu_batch import oracle_records, same

pytestmark = pytest.mark.gpu
T = ac.AhoCorasick.BATCH_TILE_BYTES
ROWS, DFA, CNFA = 3, 1, 2
_rng = np.random.default_rng(77)
_fill = lambda n: bytes(_rng.choice(np.frombuffer(b"bcfhijklmo", dtype=np.uint8), size=n))
P300 = _fill(5) + b"app" + _fill(292)   # longer than a lane's chunk; holds a short pattern that ends 292 bytes before it does
P1100 = _fill(1100)                     # its warm-up is beyond what a window's tile holds: the host form
PATS = [b"app", b"append", b"appendage", b"ndag", P300]
W = (T - ((len(P300) - 1 + 30) & ~15)) & ~63   # batch_long_window (host/engine_plan.hpp): match ends a wave owns per tile
C = W // 64
LONG_LENS = [2 * T + 1, 3 * W - 1, 3 * W, 3 * W + 1, 6 * W + 5]
N_LONG = 14
STEPPERS = {"rows": ("dfa", {}, ROWS), "dfa": ("dfa", {"batch_rows": 0}, DFA), "cnfa": ("cnfa", {}, CNFA)}


@functools.lru_cache(maxsize=None)
def planted():
    """14 long segments, two short ones in front of each; long segment j has plant category j % 7 and length LONG_LENS[j % 5]."""
    rng = np.random.default_rng(13)
    lens, cat = [], {}
    for j in range(N_LONG):
        lens += [int(rng.integers(40, 91)), int(rng.integers(40, 91)), LONG_LENS[j % 5]]
        cat[len(lens) - 1] = j % 7
    off = 3 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    hay = rng.integers(0x71, 0x7B, size=int(off[-1]) + 11, dtype=np.uint8)   # q..z: no letter of the patterns
    put = lambda pos, w: hay.__setitem__(slice(pos, pos + len(w)), np.frombuffer(w, dtype=np.uint8))
    for s, c in cat.items():
        b, e = int(off[s]), int(off[s + 1])
        if c == 0: put(b, PATS[2])                          # at the segment's first bytes
        if c == 1: put(e - 4, PATS[3])                      # at its last bytes
        if c == 2: put(b + W + 17 * C - 4, PATS[2])         # across a lane-chunk edge
        if c == 3: put(b + 2 * W - 4, PATS[2])              # across a window edge
        if c == 4: put(b - 3, PATS[1]), put(e - 2, PATS[1])  # from the previous segment's tail, and into the next one: neither is this one's
        if c == 6: put(b + 2 * W - 20, P300)                # (5: nothing)  starts in window 1 and ends in window 2; its "app" ends in window 1
    return hay, off, sorted(cat)


@functools.lru_cache(maxsize=None)
def wanted(mk, anchored, earliest, pats=tuple(PATS)):
    hay, off, _ = planted()
    _, o = build_pair(list(pats), mk, {"start_kind": "both"})
    return oracle_records(o, hay, off, anchored, earliest)


def run(a, shift, anchored=False, earliest=False):
    hay, off, _ = planted()
    buf = torch.empty(len(hay) + 5, dtype=torch.uint8, device="cuda")
    dev = buf[shift:shift + len(hay)]
    dev.copy_(torch.from_numpy(hay))
    prof = _lib.CProfile()
    return a.find_batch(dev, torch.from_numpy(off).cuda(), anchored=anchored, earliest=earliest, profile=prof), prof


@pytest.mark.parametrize("stepper", list(STEPPERS))
@pytest.mark.parametrize("anchored,earliest", [(False, False), (False, True), (True, False)])
@pytest.mark.parametrize("mk", ["standard", "leftmost_first", "leftmost_longest"])
def test_semantics_and_steppers(mk, anchored, earliest, stepper):
    hay, off, longs = planted()
    want = wanted(mk, anchored, earliest)
    lw = want[longs]
    lb, le = off[longs].astype(np.uint64), off[np.array(longs) + 1].astype(np.uint64)
    hit = lw["pattern"] != ac.NO_MATCH
    assert (~hit).sum() >= 2 and np.count_nonzero(hit & (lw["start"] == lb)) >= 2
    if not anchored:
        assert np.count_nonzero(hit & (lw["end"] == le)) >= 2
        if mk != "standard" and not earliest:   # the 300-byte pattern wins over its "app", which ends a window earlier
            sharp = hit & (lw["pattern"] == 4)
            assert sharp.sum() >= 2 and np.all((lw["end"][sharp] - 1 - lb[sharp]) // W > (lw["start"][sharp] + 8 - 1 - lb[sharp]) // W)
    kind, variants, form = STEPPERS[stepper]
    a, _ = build_pair(PATS, mk, {"kind": kind, "start_kind": "both"}, variants={"batch_lane_max": 2 * T, **variants})
    for shift in (0, 5):
        got, prof = run(a, shift, anchored, earliest)
        same(got, want, f"base+{shift}")
        assert prof.engine_used == form and prof.n_active_chunks == N_LONG and prof.routed == 0 and prof.ms_fill > 0
        assert prof.n_matches == np.count_nonzero(want["pattern"] != ac.NO_MATCH)


@pytest.mark.parametrize("mk", ["standard", "leftmost_first"])
def test_empty_pattern(mk):
    pats = PATS + [b""]
    a, _ = build_pair(pats, mk, {"start_kind": "both"}, variants={"batch_lane_max": 2 * T})
    got, prof = run(a, 5)
    same(got, wanted(mk, False, False, tuple(pats)))
    assert prof.n_active_chunks == N_LONG and prof.routed == 0 and prof.ms_fill > 0


@pytest.mark.parametrize("plant", ["last_window", "first_window", "none"])
def test_one_segment_across_the_grid(plant):
    n_bytes = (1 << 20) + 77
    hay = np.random.default_rng(3).integers(0x71, 0x7B, size=n_bytes, dtype=np.uint8)
    pos = {"last_window": n_bytes - 10 - 100, "first_window": 10 + 100}.get(plant)
    if pos is not None:
        hay[pos:pos + 9] = np.frombuffer(PATS[2], dtype=np.uint8)
    off = np.array([10, n_bytes - 10], dtype=np.int64)
    a, o = build_pair(PATS, "leftmost_first", variants={"batch_lane_max": 2 * T, "batch_blocks": 2})
    want = oracle_records(o, hay, off)
    assert (want["pattern"][0] == ac.NO_MATCH) == (pos is None)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out = torch.full((24 + 32,), 0x5A, dtype=torch.uint8, device="cuda")
        prof = _lib.CProfile()
        a.find_batch(torch.from_numpy(hay).cuda(), torch.from_numpy(off).cuda(), out=out[16:], profile=prof)
        stream.synchronize()
        host = out.cpu().numpy()
    same(host[16:40].view(ac.MATCH_DTYPE), want)
    assert np.all(host[:16] == 0x5A) and np.all(host[40:] == 0x5A)
    assert prof.n_active_chunks == 1 and prof.routed == 0 and prof.n_matches == (pos is not None)


@pytest.mark.parametrize("pats,variants", [(PATS, {"batch_long": 0}), (PATS + [P1100], {})])
def test_host_form_remains(pats, variants):
    a, _ = build_pair(pats, "leftmost_first", {"start_kind": "both"}, variants={"batch_lane_max": 2 * T, **variants})
    got, prof = run(a, 0)
    same(got, wanted("leftmost_first", False, False, tuple(pats)))
    assert prof.n_active_chunks == N_LONG and prof.routed == N_LONG

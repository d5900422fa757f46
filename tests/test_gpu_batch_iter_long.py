"""-m gpu: the long segments of the batched overlapping iterator on the device (device/batch_iter_long.hip): records and
rec_off against the oracle's find_overlapping_iter over the spans (expect / check of test_gpu_batch_iter.py), with variant
batch_lane_max = 2 T so that "long" is small -- every stepper, plants on every edge of the window / lane-chunk grid, a window
beyond the staging area, an empty pattern, one segment across the grid, and the single-span calls that remain.  Integers:
equality."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import aho_corasick_amd as ac
from aho_corasick_amd import _lib
from gpu_util import build_pair
from test_gpu_batch_iter import check, expect

pytestmark = pytest.mark.gpu
T = ac.AhoCorasick.BATCH_TILE_BYTES
STAGE = ac.AhoCorasick.BATCH_ITER_STAGE
ROWS, DFA, CNFA = 3, 1, 2
_rng = np.random.default_rng(77)
_fill = lambda n: bytes(_rng.choice(np.frombuffer(b"bcfhijklmo", dtype=np.uint8), size=n))
P300 = _fill(5) + b"app" + _fill(292)   # longer than a lane's chunk; holds a short pattern
P1100 = _fill(1100)                     # its warm-up is beyond what a window's tile holds: the host form
PATS = [b"app", b"append", b"appendage", b"ndag", b"pend", P300]
W = (T - ((len(P300) - 1 + 30) & ~15)) & ~63   # batch_long_window (host/engine_plan.hpp): match ends a wave owns per tile
C = W // 64
LONG_LENS = [2 * T + 1, 3 * W - 1, 3 * W, 3 * W + 1, 6 * W + 5]
N_LONG = 14
STEPPERS = {"rows": ({"kind": "dfa"}, {}, ROWS), "dfa": ({"kind": "dfa"}, {"batch_rows": 0}, DFA),
            "cnfa": ({"kind": "cnfa", "start_kind": "both"}, {}, CNFA)}


@functools.lru_cache(maxsize=None)
def planted():
    """14 long segments, two short ones in front of each; long segment j has plant category j % 8 and length LONG_LENS[j % 5]."""
    rng = np.random.default_rng(13)
    lens, cat = [], {}
    for j in range(N_LONG):
        lens += [int(rng.integers(40, 91)), int(rng.integers(40, 91)), LONG_LENS[j % 5]]
        cat[len(lens) - 1] = j % 8
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
        if c == 6: put(b + 2 * W - 20, P300)                # (5: nothing)  starts in window 1 and ends in window 2
        if c == 7: put(b + W + 100, b"app" * 200), put(b + 40, PATS[1])   # one window beyond the staging area, one under it
    return hay, off, cat


@functools.lru_cache(maxsize=None)
def wanted(pats=tuple(PATS), overlapping=True):
    hay, off, _ = planted()
    return expect(build_pair(list(pats), "standard", {"start_kind": "both"})[1], hay, off, overlapping=overlapping)


def run(a, shift=0, overlapping=True):
    hay, off, _ = planted()
    buf = torch.empty(len(hay) + 5, dtype=torch.uint8, device="cuda")
    dev = buf[shift:shift + len(hay)]
    dev.copy_(torch.from_numpy(hay))
    prof = _lib.CProfile()
    return a.find_iter_batch(dev, torch.from_numpy(off).cuda(), overlapping=overlapping, profile=prof), prof


def on_device_form(prof, n_long=N_LONG):
    return prof.n_active_chunks == n_long and prof.routed == 0 and prof.ms_fill > 0


@pytest.mark.parametrize("shift", [0, 5])
@pytest.mark.parametrize("stepper", list(STEPPERS))
def test_plants_and_steppers(stepper, shift):
    hay, off, cat = planted()
    want = wanted()
    # the oracle's answer has every category: per long segment, its records relative to its begin
    per = {s: want[0][int(want[1][s]):int(want[1][s + 1])] for s in cat}
    rel = {s: (r["start"].astype(np.int64) - off[s], r["end"].astype(np.int64) - off[s]) for s, r in per.items()}
    assert sum(len(r) == 0 for r in per.values()) >= 3 and all(len(per[s]) == 0 for s, c in cat.items() if c in (4, 5))
    assert any((rs == 0).any() for rs, _ in rel.values()) and any((re == off[s + 1] - off[s]).any() for s, (_, re) in rel.items())
    assert any((rs // C != (re - 1) // C).any() and (rs // W == (re - 1) // W).all() for rs, re in rel.values() if len(rs))
    assert any((rs // W != (re - 1) // W).any() for rs, re in rel.values())
    assert any(((r["pattern"] == 5) & (rs // W < (re - 1) // W)).any() for r, (rs, re) in zip(per.values(), rel.values()))
    in_window = np.concatenate([np.bincount((re - 1) // W) for _, re in rel.values() if len(re)])
    assert in_window.max() > STAGE and np.count_nonzero((in_window > 0) & (in_window <= STAGE)) >= 5
    kw, variants, form = STEPPERS[stepper]
    a, _ = build_pair(PATS, "standard", kw, variants={"batch_lane_max": 2 * T, **variants})
    got, prof = run(a, shift)
    check(got, want, f"base+{shift}")
    assert prof.engine_used == form and on_device_form(prof) and prof.n_matches == len(want[0])


@pytest.mark.parametrize("rows", [1, 0])
def test_empty_pattern(rows):
    hay, off, cat = planted()
    pats = PATS + [b""]
    want = wanted(tuple(pats))
    for s in cat:   # a record at every position of every long segment, both ends included
        r = want[0][int(want[1][s]):int(want[1][s + 1])]
        assert np.array_equal(np.unique(r["end"][r["start"] == r["end"]]), np.arange(off[s], off[s + 1] + 1, dtype=np.uint64))
    a, _ = build_pair(pats, "standard", {"kind": "dfa"}, variants={"batch_lane_max": 2 * T, "batch_rows": rows})
    got, prof = run(a, 5)
    check(got, want)
    assert on_device_form(prof)


def test_one_segment_across_the_grid():
    n_bytes = (1 << 20) + 77
    hay = np.random.default_rng(3).integers(0x71, 0x7B, size=n_bytes, dtype=np.uint8)
    for pos in list(range(10, n_bytes - 20, 50021)) + [n_bytes - 19, 10 + 9 * W - 4]:
        hay[pos:pos + 9] = np.frombuffer(PATS[2], dtype=np.uint8)
    off = np.array([10, n_bytes - 10], dtype=np.int64)
    a, o = build_pair(PATS, "standard", variants={"batch_lane_max": 2 * T, "batch_blocks": 2})
    want = expect(o, hay, off, overlapping=True)
    total = len(want[0])
    assert total > 3 * 20 and want[0]["start"][0] == 10 and want[0]["end"][-1] == n_bytes - 10
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev, doff = torch.from_numpy(hay).cuda(), torch.from_numpy(off).cuda()
        rec = torch.zeros(2, dtype=torch.int64, device="cuda")
        out = torch.full((24 * total + 32,), 0x5A, dtype=torch.uint8, device="cuda")
        assert a.find_iter_batch(dev, doff, overlapping=True, out=out[16:16 + 24 * (total - 1)], rec_offsets=rec) == (total, False)
        stream.synchronize()
        assert bool((out == 0x5A).all())
        prof = _lib.CProfile()
        assert a.find_iter_batch(dev, doff, overlapping=True, out=out[16:16 + 24 * total], rec_offsets=rec, profile=prof) == (total, True)
        stream.synchronize()
        host = out.cpu().numpy()
    check((host[16:16 + 24 * total].view(ac.MATCH_DTYPE), rec.cpu().numpy()), want)
    assert np.all(host[:16] == 0x5A) and np.all(host[16 + 24 * total:] == 0x5A) and on_device_form(prof, 1)
    check(a.find_iter_batch(hay, off.astype(np.uint64), overlapping=True), want, "host")


@pytest.mark.parametrize("pats,variants,overlapping", [(PATS, {"batch_long": 0}, True), (PATS + [P1100], {}, True), (PATS, {}, False)])
def test_host_form_remains(pats, variants, overlapping):
    a, _ = build_pair(pats, "standard", {"start_kind": "both"}, variants={"batch_lane_max": 2 * T, **variants})
    got, prof = run(a, 0, overlapping)
    check(got, wanted(tuple(pats), overlapping))
    assert prof.n_active_chunks == N_LONG and prof.routed == N_LONG


def test_guard_flavour_stays_inside_the_hull():
    """The bounds-checked library (its own process: the flavour is chosen at load) over long segments at a misaligned base,
    both passes: no haystack access outside the aligned hull."""
    code = ("import numpy as np, torch, aho_corasick_amd as ac\n"
            "T = ac.AhoCorasick.BATCH_TILE_BYTES\n"
            "lens = np.array([0, 1, 17, 2 * T + 1, 64, 3 * T - 1, T + 1, 5 * T + 3] * 3)\n"
            "off = torch.from_numpy(5 + np.concatenate([[0], np.cumsum(lens)])).cuda()\n"
            "hay = torch.from_numpy(np.frombuffer(b'xabcabcdeab' * (int(off[-1]) // 11 + 2), dtype=np.uint8).copy()).cuda()[3:int(off[-1]) + 11]\n"
            "a = ac.AhoCorasick.builder().gpu_variant('batch_lane_max', 2 * T).build([b'abcdeabcabcdd', b'ab', b'cde'])\n"
            "p = ac._lib.CProfile()\n"
            "print('records', len(a.find_iter_batch(hay, off, overlapping=True, profile=p)[0]), p.n_active_chunks, p.routed)\n"
            "print('violations', ac.load_library().acgpu_guard_violations())\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ACGPU_LIB=os.path.join(root, "aho-corasick_amd", "lib", "libacgpu_guard.so"), PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = [l.split() for l in r.stdout.splitlines() if l.startswith(("records", "violations"))]
    assert len(out) == 2 and int(out[0][1]) > 10000 and out[0][2:] == ["9", "0"] and out[1] == ["violations", "0"], r.stdout

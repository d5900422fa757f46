"""-m gpu: batched find (acgpu_find_batch / AhoCorasick.find_batch, device/batch_find.hip): record s of a packed haystack
against the oracle's find on the span (off[s], off[s+1]) -- every stepper (LDS rows, global DFA, global contiguous NFA),
every match kind, anchored and earliest modes, segments around every tile and wavefront edge, long segments served by
acgpu_find, device-resident output.  Integers: equality."""
import functools

import numpy as np
import pytest
import torch

import aho_corasick_amd as ac
from aho_corasick_amd import _lib
from gpu_util import build_pair
from oracle import orc

pytestmark = pytest.mark.gpu
T = ac.AhoCorasick.BATCH_TILE_BYTES
ROWS, DFA, CNFA = 3, 1, 2
LENS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5]
WORDS = [b"app", b"append", b"appendage", b"ndag", b"e t"]


def small_set():   # the nested and duplicated 1-4 byte patterns over {a,b,c} of test_gpu_count.small_set
    rng = np.random.default_rng(31)
    return [bytes(rng.choice(np.frombuffer(b"abc", dtype=np.uint8), size=int(rng.integers(1, 5)))) for _ in range(14)] + [b"a", b"a"]


# the small set finds its first match within a few bytes; the second set is rare enough (4^-8 per position) for lanes to
# carry their state across tiles, and for some of the long segments to have no match at all
SETS = {"small": small_set(), "rare": [b"abcdabcd", b"ddddcccc", b"badcbadc"]}


def oracle_records(o, hay, off, anchored=False, earliest=False):
    want = np.zeros(len(off) - 1, dtype=ac.MATCH_DTYPE)
    want["pattern"] = ac.NO_MATCH
    for s in range(len(off) - 1):
        m = o.find(hay, span=(int(off[s]), int(off[s + 1])), anchored=anchored, earliest=earliest)
        if m is not None:
            want[s] = (m[0], 0, m[1], m[2])
    return want


def same(got, want, ctx=""):
    for f in ("pattern", "_pad", "start", "end"):
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(got) == len(want) and not len(bad), f"{ctx}: segment {bad[0]}: got {got[bad[0]]} want {want[bad[0]]}"


@functools.lru_cache(maxsize=None)
def geometry(n, name, kind, start_kind):
    lens = [LENS[i % len(LENS)] for i in range(n)]
    lens[-1] = lens[min(1, n - 1)] = 0   # empty first and last segments, two consecutive empty ones
    off = 3 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)   # unowned bytes in front ...
    hay = orc.gen_haystack(0, int(off[-1]) + 11, seed=0xAC02, lo=0x61, span=4)   # ... and behind
    _, o = build_pair(SETS[name], "standard", {"kind": kind, "start_kind": start_kind})
    return hay, off, oracle_records(o, hay, off)


# (a contiguous NFA with an unanchored start is walked through the DFA the device derives from it; StartKind::Both has none)
@pytest.mark.parametrize("kind,start_kind", [("dfa", "unanchored"), ("cnfa", "unanchored"), ("cnfa", "both")])
@pytest.mark.parametrize("rows", [1, 0])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 64 * 16 + 1, 64 * 16 * 3 + 7])
def test_geometry(n, rows, kind, start_kind):
    form = CNFA if start_kind == "both" else (ROWS if rows else DFA)
    for name in SETS:
        hay, off, want = geometry(n, name, kind, start_kind)
        # (the largest count on two workgroups: every wavefront takes several tasks)
        a, _ = build_pair(SETS[name], "standard", {"kind": kind, "start_kind": start_kind},
                          variants={"batch_rows": rows, "batch_blocks": 2 if n > 3000 else 0})
        doff = torch.from_numpy(off).cuda()
        buf = torch.empty(len(hay) + 5, dtype=torch.uint8, device="cuda")
        for k in (0, 1, 5):   # an aligned and two misaligned bases
            dev = buf[k:k + len(hay)]
            dev.copy_(torch.from_numpy(hay))
            prof = _lib.CProfile()
            same(a.find_batch(dev, doff, profile=prof), want, f"{name} base+{k}")
            assert prof.engine_used == form and prof.n_chunks == (n + 63) // 64 and prof.n_active_chunks == 0
            assert prof.n_matches == np.count_nonzero(want["pattern"] != ac.NO_MATCH)
        same(a.find_batch(hay, off.astype(np.uint64)), want, f"{name} host")
        if name == "rare" and n > 64:
            assert 0 < np.count_nonzero(want["pattern"] != ac.NO_MATCH) < n


@functools.lru_cache(maxsize=None)
def planted():
    """~2 000 segments of 20..90 random lower-case bytes (every 64th empty) with WORDS planted at segment starts, at segment
    ends, inside, and across segment boundaries."""
    rng = np.random.default_rng(5)
    lens = rng.integers(20, 91, size=2000)
    lens[63::64] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    hay = rng.integers(0x61, 0x7B, size=int(off[-1]), dtype=np.uint8)
    for s in range(0, 2000 - 16, 16):
        for pos, w in ((off[s], WORDS[1]), (off[s + 5] - 4, WORDS[3]), (off[s + 9] - 4, WORDS[2]), (off[s + 12] + 7, WORDS[4])):
            hay[pos:pos + len(w)] = np.frombuffer(w, dtype=np.uint8)
    return hay, off


SEMANTICS = [(mk, anchored, earliest, kind, {}) for mk in ("standard", "leftmost_first", "leftmost_longest")
             for anchored, kind in ((False, None), (True, "dfa"), (True, None)) for earliest in (False, True)]
SEMANTICS += [("standard", False, False, None, {"empty": True}), ("leftmost_first", False, False, None, {"casei": True})]


@pytest.mark.parametrize("mk,anchored,earliest,kind,extra", SEMANTICS)
def test_semantics(mk, anchored, earliest, kind, extra):
    hay, off = planted()
    pats = WORDS + [b""] if extra.get("empty") else WORDS
    if extra.get("casei"):
        hay = hay - 32 * (np.arange(len(hay)) % 3 == 0).astype(np.uint8)   # every third letter in upper case
    kw = {"kind": kind, "start_kind": "both" if anchored else "unanchored", "ascii_case_insensitive": bool(extra.get("casei"))}
    a, o = build_pair(pats, mk, kw)
    want = oracle_records(o, hay, off, anchored, earliest)
    hit = want["pattern"] != ac.NO_MATCH
    if extra.get("empty"):   # the empty pattern matches at the start of every segment, empty ones included
        assert hit.all() and np.array_equal(want["start"], off[:-1].astype(np.uint64)) and np.array_equal(want["end"], want["start"])
    else:
        assert hit.sum() >= 100 and (~hit).sum() >= 100
        assert np.count_nonzero(hit & (want["start"] == off[:-1].astype(np.uint64))) >= 20
    if not anchored and not extra:
        assert np.count_nonzero(hit & (want["end"] == off[1:].astype(np.uint64))) >= 20
        occ = orc.Oracle(WORDS).find_overlapping_iter(hay, as_numpy=True)   # over the whole buffer: occurrences across boundaries
        nxt = off[np.searchsorted(off, occ["start"].astype(np.int64), side="right").clip(max=len(off) - 1)]
        assert np.count_nonzero(nxt < occ["end"].astype(np.int64)) >= 20
        assert np.all(want["start"][hit] >= off[:-1][hit].astype(np.uint64)) and np.all(want["end"][hit] <= off[1:][hit].astype(np.uint64))
    prof = _lib.CProfile()
    got = a.find_batch(torch.from_numpy(hay).cuda(), torch.from_numpy(off).cuda(), anchored=anchored, earliest=earliest, profile=prof)
    same(got, want)
    assert prof.engine_used == (CNFA if anchored and kind is None else ROWS)


def test_long_segments_are_served_by_find():
    pats = [b"appendage", b"append", b"app", b"ndag"]   # leftmost-first: "app" is reached first, "appendage" is the answer
    rng = np.random.default_rng(11)
    lens = rng.integers(30, 61, size=203)
    lens[[50, 100, 150]] = [2 * T + 1, 5 * T, 2 * T]   # just over the limit, far over it, exactly at it
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    hay = rng.integers(0x71, 0x7B, size=int(off[-1]), dtype=np.uint8)   # q..z: no letter of the patterns
    for s in (7, 50, 100, 150, 190):
        pos = off[s] + lens[s] // 2
        hay[pos:pos + 9] = np.frombuffer(pats[0], dtype=np.uint8)
    a, o = build_pair(pats, "leftmost_first", variants={"batch_lane_max": 2 * T})
    want = oracle_records(o, hay, off)
    assert all(want["pattern"][s] == 0 and want["end"][s] - want["start"][s] == 9 for s in (7, 50, 100, 150, 190))
    prof = _lib.CProfile()
    same(a.find_batch(torch.from_numpy(hay).cuda(), torch.from_numpy(off).cuda(), profile=prof), want)
    assert prof.n_active_chunks == 2 and prof.n_matches == np.count_nonzero(want["pattern"] != ac.NO_MATCH)
    same(a.find_batch(hay, off), want, "host")


def test_device_output_on_a_side_stream():
    hay, off = planted()
    n = len(off) - 1
    a, o = build_pair(WORDS, "leftmost_longest")
    want = oracle_records(o, hay, off)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev, doff = torch.from_numpy(hay).cuda(), torch.from_numpy(off).cuda()
        for shift in (0, 8):   # a 16-byte aligned record buffer, and one that is not
            out = torch.full((24 * n + 48,), 0x5A, dtype=torch.uint8, device="cuda")
            view = out[shift:]
            assert a.find_batch(dev, doff, out=view) is view
            stream.synchronize()
            host = out.cpu().numpy()
            same(host[shift:shift + 24 * n].view(ac.MATCH_DTYPE), want, f"shift {shift}")
            assert np.all(host[:shift] == 0x5A) and np.all(host[shift + 24 * n:] == 0x5A)
        bad = doff.clone()
        bad[1000] = bad[1001] + 1   # device offsets are validated on the device
        with pytest.raises(RuntimeError, match=r"offsets\[1001\]"):
            a.find_batch(dev, bad)

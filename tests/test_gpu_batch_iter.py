"""-m gpu: batched iterator (acgpu_find_iter_batch / AhoCorasick.find_iter_batch, device/batch_iter.hip): the records of a
packed haystack against the concatenation of the oracle's find_iter (overlapping: find_overlapping_iter) over the spans
(off[s], off[s+1]), rec_off against its running count.  Integers: equality."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import aho_corasick_amd as ac
from aho_corasick_amd import _lib
from gpu_util import assert_same, build_pair
from oracle import orc
from test_gpu_batch import LENS, SETS

pytestmark = pytest.mark.gpu
T = ac.AhoCorasick.BATCH_TILE_BYTES
STAGE = ac.AhoCorasick.BATCH_ITER_STAGE
ROWS, DFA, CNFA = 3, 1, 2
WORDS = [b"app", b"append", b"appendage", b"ndag", b"e t", b"pend"]   # ("append" and "pend" end together)


def expect(o, hay, off, anchored=False, earliest=False, overlapping=False):
    spans = [(int(b), int(e)) for b, e in zip(off[:-1], off[1:])]
    if overlapping:
        parts = [o.find_overlapping_iter(hay, span=s, anchored=anchored, as_numpy=True) for s in spans]
    else:
        parts = [o.find_iter(hay, span=s, anchored=anchored, earliest=earliest, as_numpy=True) for s in spans]
    return np.concatenate(parts), np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)


def check(got, want, ctx=""):
    assert np.array_equal(np.asarray(got[1]).astype(np.uint64), want[1]), f"{ctx}: rec_off"
    assert_same(got[0], want[0], ctx)
    assert not got[0]["_pad"].any()


def on_device(a, hay, off, total, **kw):
    """the device form with a record buffer of exactly `total` records: (records, rec_off) read back"""
    dev, doff = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (hay, off.astype(np.int64)))
    rec = torch.zeros(len(off), dtype=torch.int64, device="cuda")
    out = torch.empty(24 * total, dtype=torch.uint8, device="cuda")
    assert a.find_iter_batch(dev, doff, out=out, rec_offsets=rec, **kw) == (total, True)
    return out.cpu().numpy().view(ac.MATCH_DTYPE), rec.cpu().numpy()


@functools.lru_cache(maxsize=None)
def geometry(n, name):
    lens = [LENS[i % len(LENS)] for i in range(n)]
    lens[-1] = lens[min(1, n - 1)] = 0   # empty first and last segments
    off = 3 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)   # unowned bytes in front ...
    hay = orc.gen_haystack(0, int(off[-1]) + 11, seed=0xAC02, lo=0x61, span=4)   # ... and behind
    return hay, off, expect(orc.Oracle(SETS[name]), hay, off)


@pytest.mark.parametrize("kind,start_kind", [("dfa", "unanchored"), ("cnfa", "unanchored"), ("cnfa", "both")])
@pytest.mark.parametrize("rows", [1, 0])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 64 * 16 + 1])
def test_geometry(n, rows, kind, start_kind):
    form = CNFA if start_kind == "both" else (ROWS if rows else DFA)
    for name in SETS:
        hay, off, want = geometry(n, name)
        per_task = np.diff(want[1][np.r_[0:n:64, n]].astype(np.int64))
        if n >= 63:   # the dense set overflows the staging area (direct store), the rare one stays under it (staged store)
            assert per_task.max() > STAGE if name == "small" else 0 < per_task.max() <= STAGE
        a, _ = build_pair(SETS[name], "standard", {"kind": kind, "start_kind": start_kind},
                          variants={"batch_rows": rows, "batch_blocks": 2 if n > 1000 else 0})
        buf = torch.empty(len(hay) + 5, dtype=torch.uint8, device="cuda")
        for k in (0, 1, 5):   # an aligned and two misaligned bases
            dev = buf[k:k + len(hay)]
            dev.copy_(torch.from_numpy(hay))
            prof = _lib.CProfile()
            check(a.find_iter_batch(dev, torch.from_numpy(off).cuda(), profile=prof), want, f"{name} base+{k}")
            assert prof.engine_used == form and prof.n_chunks == (n + 63) // 64 and prof.n_active_chunks == 0
            assert prof.n_matches == len(want[0])
        check(a.find_iter_batch(hay, off.astype(np.uint64)), want, f"{name} host")
        check(on_device(a, hay, off, len(want[0])), want, f"{name} device output")


@functools.lru_cache(maxsize=None)
def planted():
    """~2 000 segments of 20..90 random lower-case bytes (every 64th empty), words at segment starts (adjacent ones too: an
    anchored iteration finds its second match only where the first one ends), at segment ends, inside, and across boundaries."""
    rng = np.random.default_rng(5)
    lens = rng.integers(20, 91, size=2000)
    lens[63::64] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    hay = rng.integers(0x61, 0x7B, size=int(off[-1]), dtype=np.uint8)
    for s in range(0, 2000 - 16, 16):
        for pos, w in ((off[s], WORDS[1]), (off[s] + 10, WORDS[3]), (off[s + 2], b"appapp"), (off[s + 3], b"appendpend"),
                       (off[s + 5] - 4, WORDS[3]), (off[s + 9] - 4, WORDS[2]),
                       (off[s + 12] + 7, WORDS[4]), (off[s + 12] + 11, WORDS[2])):
            hay[pos:pos + len(w)] = np.frombuffer(w, dtype=np.uint8)
    return hay, off


SEMANTICS = [(mk, anchored, earliest, kind, {}) for mk in ("standard", "leftmost_first", "leftmost_longest")
             for anchored, kind in ((False, None), (True, "dfa"), (True, None)) for earliest in (False, True)]
SEMANTICS += [("standard", False, False, None, {"empty": True}), ("leftmost_first", False, False, None, {"casei": True})]
# (the reference refuses anchored overlapping iteration: tests/test_batch_iter_args.py)
SEMANTICS += [("standard", False, False, "dfa", {"ovl": True, "empty": empty, "rows": rows}) for empty in (False, True) for rows in (1, 0)]
SEMANTICS += [("standard", False, False, None, {"ovl": True, "both": True})]   # StartKind::Both: the contiguous NFA's match lists


@pytest.mark.parametrize("mk,anchored,earliest,kind,extra", SEMANTICS)
def test_semantics(mk, anchored, earliest, kind, extra):
    """The oracle's answer has at least 100 segments without a record and 100 with two or more, and, overlapping, 20
    positions with several patterns."""
    hay, off = planted()
    ovl = bool(extra.get("ovl"))
    pats = WORDS + [b""] if extra.get("empty") else WORDS
    if extra.get("casei"):
        hay = hay - 32 * (np.arange(len(hay)) % 3 == 0).astype(np.uint8)   # every third letter in upper case
    kw = {"kind": kind, "start_kind": "both" if anchored or extra.get("both") else "unanchored", "ascii_case_insensitive": bool(extra.get("casei"))}
    a, o = build_pair(pats, mk, kw, variants={"batch_rows": extra.get("rows", 1)})
    want = expect(o, hay, off, anchored, earliest, ovl)
    per_seg = np.diff(want[1].astype(np.int64))
    if extra.get("empty"):   # a record at every position of every segment, empty segments included
        idx = np.nonzero(want[0]["start"] == want[0]["end"])[0]
        seg, at = np.searchsorted(want[1], idx, side="right") - 1, want[0]["end"][idx].astype(np.int64)
        assert np.all((at >= off[seg]) & (at <= off[seg + 1]))
        assert np.unique(np.stack([seg, at]), axis=1).shape[1] == int(np.sum(np.diff(off) + 1))
    else:
        assert np.count_nonzero(per_seg >= 2) >= 100 and np.count_nonzero(per_seg == 0) >= 100
    if ovl:
        ends, cnt = np.unique(want[0]["end"][want[0]["end"] > want[0]["start"]], return_counts=True)
        assert np.count_nonzero(cnt > 1) >= 20
    prof = _lib.CProfile()
    got = a.find_iter_batch(torch.from_numpy(hay).cuda(), torch.from_numpy(off).cuda(), anchored=anchored, earliest=earliest,
                            overlapping=ovl, profile=prof)
    check(got, want)
    assert prof.engine_used == (CNFA if (anchored or extra.get("both")) and kind is None else ROWS if extra.get("rows", 1) else DFA)


@pytest.mark.parametrize("n", [1, 64])
def test_restart_behind_the_tile(n):
    long_pat = b"ab" + b"qrstuv" + b"ab" + bytes(range(0x30, 0x30 + 30))   # 40 bytes; b"ab" again at offset 8
    lens = [2 * T + 100] + [10] * (n - 1)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    hay = np.full(int(off[-1]), 0x2E, dtype=np.uint8)
    hay[T - 6:T + 20] = np.frombuffer(long_pat[:26], dtype=np.uint8)   # "ab" ends 4 bytes in front of T; the prefix breaks at T + 20
    hay[off[1:-1:7] + 3] = 0x61
    hay[off[1:-1:7] + 4] = 0x62
    a, o = build_pair([long_pat, b"ab"], "leftmost_first")
    want = expect(o, hay, off)
    assert [tuple(r)[2:] for r in want[0][:2]] == [(T - 6, T - 4), (T + 2, T + 4)] and all(want[0]["pattern"] == 1)
    check(a.find_iter_batch(torch.from_numpy(hay).cuda(), torch.from_numpy(off).cuda()), want)


@pytest.mark.parametrize("ovl", [False, True])
def test_long_segments_are_served_by_the_single_span_calls(ovl):
    pats = [b"append", b"app", b"ndag", b"pend"]
    rng = np.random.default_rng(11)
    lens = rng.integers(30, 61, size=203)
    lens[[7, 50, 100, 150, 190]] = [60, 2 * T + 1, 5 * T, 2 * T, 60]   # just over the limit, far over it, exactly at it
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    hay = rng.integers(0x71, 0x7B, size=int(off[-1]), dtype=np.uint8)   # q..z: no letter of the patterns
    for s in (7, 50, 100, 150, 190):
        for pos in (off[s] + 2, off[s] + lens[s] // 2, off[s + 1] - 10):
            hay[pos:pos + 9] = np.frombuffer(b"appendage", dtype=np.uint8)
    a, o = build_pair(pats, "standard", variants={"batch_lane_max": 2 * T})
    want = expect(o, hay, off, overlapping=ovl)
    assert all(np.diff(want[1].astype(np.int64))[s] >= 6 for s in (7, 50, 100, 150, 190))
    prof = _lib.CProfile()
    check(a.find_iter_batch(torch.from_numpy(hay).cuda(), torch.from_numpy(off).cuda(), overlapping=ovl, profile=prof), want)
    assert prof.n_active_chunks == 2 and prof.n_matches == len(want[0])
    check(a.find_iter_batch(hay, off, overlapping=ovl), want, "host")
    check(on_device(a, hay, off, len(want[0]), overlapping=ovl), want, "device output")


def test_device_output_and_capacity_on_a_side_stream():
    hay, off = planted()
    a, o = build_pair(WORDS, "leftmost_longest")
    want = expect(o, hay, off)
    total = len(want[0])
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dev, doff = torch.from_numpy(hay).cuda(), torch.from_numpy(off).cuda()
        rec = torch.zeros(len(off), dtype=torch.int64, device="cuda")
        for shift in (0, 8):   # a 16-byte aligned record buffer, and one that is not
            out = torch.full((24 * total + 48,), 0x5A, dtype=torch.uint8, device="cuda")
            assert a.find_iter_batch(dev, doff, out=out[shift:shift + 24 * (total - 1)], rec_offsets=rec) == (total, False)
            stream.synchronize()
            assert bool((out == 0x5A).all())
            assert a.find_iter_batch(dev, doff, out=out[shift:shift + 24 * total], rec_offsets=rec) == (total, True)
            stream.synchronize()
            host = out.cpu().numpy()
            check((host[shift:shift + 24 * total].view(ac.MATCH_DTYPE), rec.cpu().numpy()), want, f"shift {shift}")
            assert np.all(host[:shift] == 0x5A) and np.all(host[shift + 24 * total:] == 0x5A)
        bad = doff.clone()
        bad[1000] = bad[1001] + 1   # device offsets are validated on the device
        with pytest.raises(RuntimeError, match=r"offsets\[1001\]"):
            a.find_iter_batch(dev, bad)


def test_guard_flavour_stays_inside_the_hull():
    """The bounds-checked library (its own process: the flavour is chosen at load) over ragged segments at a misaligned
    base, both passes, both modes, a restart behind the tile included: no haystack access outside the aligned hull."""
    code = ("import numpy as np, torch, aho_corasick_amd as ac\n"
            "T = ac.AhoCorasick.BATCH_TILE_BYTES\n"
            "lens = np.array(([0, 1, 17, 64, T - 1, T + 1, 2 * T + 100] * 30)[:200])\n"
            "off = torch.from_numpy(5 + np.concatenate([[0], np.cumsum(lens)])).cuda()\n"
            "hay = torch.from_numpy(np.frombuffer(b'xabcabcdeab' * (int(off[-1]) // 11 + 2), dtype=np.uint8).copy()).cuda()[3:int(off[-1]) + 11]\n"
            "for mk, ovl in ((0, False), (0, True), (1, False)):\n"
            "    a = ac.AhoCorasick.builder().match_kind(mk).build([b'abcdeabcabcdd', b'ab', b'cde'])\n"
            "    print('records', len(a.find_iter_batch(hay, off, overlapping=ovl)[0]))\n"
            "print('violations', ac.load_library().acgpu_guard_violations())\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ACGPU_LIB=os.path.join(root, "aho-corasick_amd", "lib", "libacgpu_guard.so"), PYTHONPATH=root)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = [l.split() for l in r.stdout.splitlines() if l.startswith(("records", "violations"))]
    assert len(out) == 4 and all(int(v) > 1000 for k, v in out[:3]) and out[3] == ["violations", "0"], r.stdout

#!/usr/bin/env python3
"""Batched find (AhoCorasick.find_batch, device/batch_find.hip) on device-resident inputs, records left on the device:
  lines-6words   the lines of the prose corpus as segments x a 6-word set (LDS rows)
  lines-dict     the same segments x the reference's words-5000 dictionary (global stepper)
  fixed128       128-byte segments of the Appendix-C text x the headline set, variant batch_rows = 0 and automatic
  one-percent    128-byte segments, every 100th one longer than batch_lane_max: on the device (device/batch_long.hip), and
                 with variant batch_long = 0 by one acgpu_find call each
  all-long       the same text cut into 40 KiB segments, both forms
  one-huge       1, 8 and 64 MiB of the same text as ONE segment, both forms, beside a plain find call on the span;
                 one-huge-no-match: the same with a one-word set that the text does not hold
  loop           the yardstick: one find call per segment over the first 4 096 lines, against one find_batch call
  chunked-walk   ms_scan of the rows form against k_lw_count (the chunked LDS walk) over the same bytes
Per row: GB/s of packed bytes and segments/s of the whole call (host clock, median of alternating rounds after a warm-up),
and ms_scan (device events) beside it.  One JSON line per measurement."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import aho_corasick_amd as ac
from aho_corasick_amd import _lib
import corpora

ap = argparse.ArgumentParser()
ap.add_argument("--mib", type=int, default=64)
ap.add_argument("--steps", type=int, default=10)
args = ap.parse_args()
N = args.mib << 20
WORDS6 = [b"Sherlock", b"Holmes", b"Watson", b"London", b"which", b"the "]
prof = _lib.CProfile()
SPREAD = {}


def build(pats, kind=None, engine="auto", **variants):
    b = ac.AhoCorasick.builder().kind(kind).gpu_engine(engine)
    for k, v in variants.items():
        b.gpu_variant(k, v)
    return b.build(pats)


def wall(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(fns, steps):
    """fns: {label: callable returning ms}: warm-up, then the labels in turn -> {label: median ms}"""
    for f in fns.values():
        f()
    ms = {k: [] for k in fns}
    for _ in range(steps):
        for k, f in fns.items():
            ms[k].append(f())
    SPREAD.update({k: (min(v), max(v)) for k, v in ms.items()})   # the run-to-run spread of the rounds
    return {k: float(np.median(v)) for k, v in ms.items()}


def row(name, auts, buf, off, **extra):
    """auts: {label: automaton}, timed in turn; their records are compared first"""
    n, nbytes = off.numel() - 1, int(off[-1] - off[0])
    out = torch.empty(24 * n, dtype=torch.uint8, device="cuda")
    ref = None
    for label, a in auts.items():
        got = a.find_batch(buf, off, out=out, profile=prof).cpu().numpy().copy()
        assert ref is None or np.array_equal(got, ref), (name, label)
        ref = got
    scan = {}

    def call(label, a):
        def f():
            ms = wall(lambda: a.find_batch(buf, off, out=out, profile=prof))
            scan[label] = (float(prof.ms_scan), int(prof.engine_used), int(prof.n_active_chunks), float(prof.ms_fill), int(prof.routed))
            return ms
        return f
    ms = alternate({label: call(label, a) for label, a in auts.items()}, args.steps)
    hits = int(np.count_nonzero(ref.view(ac.MATCH_DTYPE)["pattern"] != ac.NO_MATCH))
    for label in auts:
        print(json.dumps({"row": name, "form": label, "segments": n, "bytes": nbytes, "matching_segments": hits,
                          "call_ms": round(ms[label], 4), "ms_scan": round(scan[label][0], 4), "stepper": scan[label][1],
                          "long_segments": scan[label][2], "ms_long": round(scan[label][3], 4), "host_find_calls": scan[label][4],
                          "spread_ms": [round(x, 4) for x in SPREAD[label]], "GBps": round(nbytes / ms[label] / 1e6, 2),
                          "Msegments_per_s": round(n / ms[label] / 1e3, 2), **extra}), flush=True)
    return ms


# ---- the lines of the prose corpus
text = corpora.haystack("sherlock.txt", N)
ends = np.flatnonzero(text == 0x0A) + 1
lines_off = torch.from_numpy(np.concatenate([[0], ends]).astype(np.int64)).cuda()
prose = torch.from_numpy(text).cuda()
rows6 = build(WORDS6)
row("lines-6words", {"rows": rows6, "global": build(WORDS6, batch_rows=0)}, prose, lines_off)
row("lines-dict", {"auto": build(corpora.words("words-5000"))}, prose, lines_off)

# ---- fixed 128-byte segments of the Appendix-C text, and the same with one segment in a hundred beyond batch_lane_max
synth = ac.gen_haystack(torch.empty(N, dtype=torch.uint8, device="cuda"), offset=0, seed=0xAC02)
headline = ac.gen_patterns(1000, seed=0xAC01)
fixed = torch.arange(0, N + 1, 128, dtype=torch.int64, device="cuda")
row("fixed128", {"auto": build(headline, ac.AhoCorasickKind.DFA), "rows0": build(headline, ac.AhoCorasickKind.DFA, batch_rows=0)}, synth, fixed)
lens = np.full(N // 128, 128, dtype=np.int64)
lens[::100] = 40 << 10
mixed = np.concatenate([[0], np.cumsum(lens)])
mixed = torch.from_numpy(mixed[mixed <= N]).cuda()
dev_long, host_long = build(headline, ac.AhoCorasickKind.DFA), build(headline, ac.AhoCorasickKind.DFA, batch_long=0)
row("one-percent", {"device": dev_long, "host_calls": host_long}, synth, mixed)
row("all-long", {"device": dev_long, "host_calls": host_long}, synth, torch.arange(0, N + 1, 40 << 10, dtype=torch.int64, device="cuda"))
# (a ceiling on the device path could only hand a huge segment to the host_calls form, so that is what it has to beat;
#  match-poor text: a set of one word the text does not hold, so every window is walked)
absent = b"\x00zq\x00absent\x00"
assert absent not in bytes(synth.cpu().numpy())
for name, pats in (("one-huge", headline), ("one-huge-no-match", [absent])):
    dev_h, host_h = (dev_long, host_long) if pats is headline else (build(pats, ac.AhoCorasickKind.DFA), build(pats, ac.AhoCorasickKind.DFA, batch_long=0))
    for size in sorted({min(N, m << 20) for m in (1, 8, 64)}):
        huge = torch.tensor([0, size], dtype=torch.int64, device="cuda")
        ms = row(name, {"device": dev_h, "host_calls": host_h}, synth[:size], huge)
        find_ms = alternate({"find": lambda: wall(lambda: dev_h.find(ac.Input(synth).range(0, size)))}, args.steps)
        print(json.dumps({"row": name, "form": "single find call", "bytes": size, "call_ms": round(find_ms["find"], 4),
                          "spread_ms": [round(x, 4) for x in SPREAD["find"]], "device_over_find": round(ms["device"] / find_ms["find"], 2),
                          "device_over_host_calls": round(ms["device"] / ms["host_calls"], 2)}), flush=True)

# ---- the yardstick: a loop of find calls over 4 096 segments (what a caller had before) against one batch call
k = 4096
host_off = lines_off[:k + 1].cpu().numpy()


def loop():
    for s in range(k):
        rows6.find(ac.Input(prose).range(int(host_off[s]), int(host_off[s + 1])))


ms = alternate({"find_loop": lambda: wall(loop), "find_batch": lambda: wall(lambda: rows6.find_batch(prose, lines_off[:k + 1]))}, 3)
print(json.dumps({"row": "loop", "segments": k, "bytes": int(host_off[-1]), "find_loop_ms": round(ms["find_loop"], 3),
                  "find_batch_ms": round(ms["find_batch"], 4), "ratio_loop_over_batch": round(ms["find_loop"] / ms["find_batch"], 1)}), flush=True)

# ---- lane-per-segment against the chunked LDS walk (k_lw_count: count walk without events) over the same bytes
walk = build(WORDS6, ac.AhoCorasickKind.DFA, "hot", lw_events=0)


def scan_batch():
    rows6.find_batch(prose, lines_off, out=scratch, profile=prof)
    return float(prof.ms_scan)


def scan_walk():
    walk.overlapping_device(prose, out=None, profile=prof)
    return float(prof.ms_scan)


scratch = torch.empty(24 * (lines_off.numel() - 1), dtype=torch.uint8, device="cuda")
ms = alternate({"batch_rows": scan_batch, "k_lw_count": scan_walk}, args.steps)
print(json.dumps({"row": "chunked-walk", "bytes": N, "batch_rows_scan_ms": round(ms["batch_rows"], 4), "k_lw_count_scan_ms": round(ms["k_lw_count"], 4),
                  "ratio_batch_over_walk": round(ms["batch_rows"] / ms["k_lw_count"], 2)}), flush=True)

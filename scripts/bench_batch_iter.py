#!/usr/bin/env python3
"""Batched iterator (AhoCorasick.find_iter_batch, device/batch_iter.hip) on device-resident inputs, records and rec_off left
on the device: the lines of the prose corpus as segments x the 6-word set of bench_batch.py, both modes, LDS rows and
batch_rows = 0.  Per row: the whole call (host clock) with ms_compact (classify + count + prefix sum) and ms_scan (fill)
from device events, all three medians of the same alternating rounds after a warm-up (spread_ms: min and max of the rounds), beside
  find_batch   the same automaton's first-match call on the same input: the floor that one pass over first matches costs
  loop         the yardstick: one find_iter / find_overlapping_iter call per line over the first 4 096 lines, against one
               find_iter_batch call over them
and, overlapping, two layouts with segments beyond batch_lane_max over the Appendix-C text x the headline set (bench_batch.py's):
  one-percent  128-byte segments, every 100th one of 40 KiB: on the device (device/batch_iter_long.hip), and with variant
               batch_long = 0 by one acgpu_find_overlapping call each
  all-long     the same text cut into 40 KiB segments, both forms
with ms_fill (the long-segment launches, device events) and the number of single-span calls.  One JSON line per measurement."""
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


def build(pats, **variants):
    b = ac.AhoCorasick.builder()
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


text = corpora.haystack("sherlock.txt", N)
ends = np.flatnonzero(text == 0x0A) + 1
lines_off = torch.from_numpy(np.concatenate([[0], ends]).astype(np.int64)).cuda()
prose = torch.from_numpy(text).cuda()
n, nbytes = lines_off.numel() - 1, int(lines_off[-1])
rec = torch.empty(n + 1, dtype=torch.int64, device="cuda")
first = torch.empty(24 * n, dtype=torch.uint8, device="cuda")
auts = {"rows": build(WORDS6), "global": build(WORDS6, batch_rows=0)}

for ovl in (False, True):
    total, _ = auts["rows"].find_iter_batch(prose, lines_off, overlapping=ovl, out=first[:0], rec_offsets=rec)
    out = torch.empty(24 * total, dtype=torch.uint8, device="cuda")
    ref, legs = None, {}
    for label, a in auts.items():   # the forms agree before they are timed
        assert a.find_iter_batch(prose, lines_off, overlapping=ovl, out=out, rec_offsets=rec) == (total, True)
        got = (out.cpu().numpy().copy(), rec.cpu().numpy().copy())
        assert ref is None or all(np.array_equal(x, y) for x, y in zip(got, ref)), label
        ref = got

    def call(label, a):
        def f():
            ms = wall(lambda: a.find_iter_batch(prose, lines_off, overlapping=ovl, out=out, rec_offsets=rec, profile=prof))
            legs.setdefault(label, []).append((float(prof.ms_compact), float(prof.ms_scan), int(prof.engine_used), float(prof.ms_fill)))
            return ms
        return f

    def floor(label, a):
        def f():
            ms = wall(lambda: a.find_batch(prose, lines_off, out=first, profile=prof))
            legs.setdefault("find_batch " + label, []).append((float(prof.ms_compact), float(prof.ms_scan), int(prof.engine_used), float(prof.ms_fill)))
            return ms
        return f
    fns = {label: call(label, a) for label, a in auts.items()}
    fns.update({"find_batch " + label: floor(label, a) for label, a in auts.items()})
    ms = alternate(fns, args.steps)
    legs = {k: tuple(np.median(np.array(v[1:]), axis=0)) for k, v in legs.items()}   # (medians of the timed rounds, as call_ms)
    with_records = int(np.count_nonzero(np.diff(ref[1])))
    for label in fns:
        print(json.dumps({"row": "lines-6words", "overlapping": ovl, "form": label, "segments": n, "bytes": nbytes, "records": total,
                          "segments_with_records": with_records, "call_ms": round(ms[label], 4), "ms_compact": round(legs[label][0], 4),
                          "ms_scan": round(legs[label][1], 4), "ms_fill": round(legs[label][3], 4), "stepper": int(legs[label][2]),
                          "spread_ms": [round(x, 4) for x in SPREAD[label]], "GBps": round(nbytes / ms[label] / 1e6, 2),
                          "Msegments_per_s": round(n / ms[label] / 1e3, 2)}), flush=True)

    # ---- the yardstick: a loop of single-span calls over 4 096 lines (what a caller had before) against one batched call
    k = 4096
    host_off = lines_off[:k + 1].cpu().numpy()
    rows6 = auts["rows"]
    one = rows6.find_overlapping_iter if ovl else rows6.find_iter

    def loop():
        for s in range(k):
            one(ac.Input(prose).range(int(host_off[s]), int(host_off[s + 1])), as_numpy=True)

    ms = alternate({"loop": lambda: wall(loop),
                    "batch": lambda: wall(lambda: rows6.find_iter_batch(prose, lines_off[:k + 1], overlapping=ovl))}, 3)
    print(json.dumps({"row": "loop", "overlapping": ovl, "segments": k, "bytes": int(host_off[-1]), "loop_ms": round(ms["loop"], 3),
                      "find_iter_batch_ms": round(ms["batch"], 4), "ratio_loop_over_batch": round(ms["loop"] / ms["batch"], 1)}), flush=True)

# ---- segments beyond batch_lane_max, overlapping: on the device against one single-span call each
synth = ac.gen_haystack(torch.empty(N, dtype=torch.uint8, device="cuda"), offset=0, seed=0xAC02)
headline = ac.gen_patterns(1000, seed=0xAC01)
lens = np.full(N // 128, 128, dtype=np.int64)
lens[::100] = 40 << 10
mixed = np.concatenate([[0], np.cumsum(lens)])
layouts = {"one-percent": torch.from_numpy(mixed[mixed <= N]).cuda(), "all-long": torch.arange(0, N + 1, 40 << 10, dtype=torch.int64, device="cuda")}
forms = {"device": build(headline), "host_calls": build(headline, batch_long=0)}
for name, off in layouts.items():
    n, nbytes = off.numel() - 1, int(off[-1] - off[0])
    rec = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    total, _ = forms["device"].find_iter_batch(synth, off, overlapping=True, out=first[:0], rec_offsets=rec)
    out = torch.empty(24 * total, dtype=torch.uint8, device="cuda")
    ref, legs = None, {}
    for label, a in forms.items():   # the forms agree before they are timed
        assert a.find_iter_batch(synth, off, overlapping=True, out=out, rec_offsets=rec) == (total, True)
        got = (out.cpu().numpy().copy(), rec.cpu().numpy().copy())
        assert ref is None or all(np.array_equal(x, y) for x, y in zip(got, ref)), (name, label)
        ref = got

    def call(label, a):
        def f():
            ms = wall(lambda: a.find_iter_batch(synth, off, overlapping=True, out=out, rec_offsets=rec, profile=prof))
            legs.setdefault(label, []).append((float(prof.ms_compact), float(prof.ms_scan), float(prof.ms_fill), int(prof.n_active_chunks), int(prof.routed)))
            return ms
        return f
    ms = alternate({label: call(label, a) for label, a in forms.items()}, args.steps)
    for label in forms:
        leg = np.median(np.array(legs[label][1:]), axis=0)
        print(json.dumps({"row": name, "overlapping": True, "form": label, "segments": n, "bytes": nbytes, "records": total,
                          "call_ms": round(ms[label], 4), "ms_compact": round(leg[0], 4), "ms_scan": round(leg[1], 4), "ms_fill": round(leg[2], 4),
                          "long_segments": int(leg[3]), "single_span_calls": int(leg[4]), "spread_ms": [round(x, 4) for x in SPREAD[label]],
                          "GBps": round(nbytes / ms[label] / 1e6, 2)}), flush=True)

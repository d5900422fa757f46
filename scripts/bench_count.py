#!/usr/bin/env python3
"""A/B of per-pattern occurrence counts (AhoCorasick.count_patterns, device/lds_hist.hip) on device-resident haystacks:
  walk      k_lw_hist against k_lw_count of the same automaton (ms_scan of the overlapping search with engine `hot`, the
            count walk without events), device events through acgpu_profile
  forms     the whole call: state visits against the records form (variant count_hist = 0), host clock around the
            synchronous call, counts left on the device
  agree     the wave-agreement shortcut of hot bins on / off (count_hist = 1 / 2), ms_scan
  old-way   the whole call against find_overlapping_iter(as_numpy=True) + np.bincount
Inputs: sparse = the headline set on the Appendix-C text; prose = English prose x a small word set (one row per state);
same = one repeated byte x nested patterns of it (a record or more per byte).  The compared forms alternate within the
process after a warm-up, and their results are compared at the timed size first.  One JSON line per measurement."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import aho_corasick_amd as ac
from aho_corasick_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--gib", type=float, default=1.0)
ap.add_argument("--old-way-mib", type=int, default=64, help="size of the old-way comparison on `same` (24 bytes per record reach the host)")
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--inputs", default="sparse,prose,same")
args = ap.parse_args()
n = int(args.gib * (1 << 30)) // 64 * 64


def inputs(name):
    buf = torch.empty(n, dtype=torch.uint8, device="cuda")
    if name == "sparse":
        ac.gen_haystack(buf, offset=0, seed=0xAC02)
        return ac.gen_patterns(1000, seed=0xAC01), buf
    if name == "prose":
        import corpora
        t = torch.from_numpy(corpora.haystack("sherlock.txt")).cuda()
        buf.copy_(t.repeat(-(-n // t.numel()))[:n])
        return [b"Sherlock", b"Holmes", b"Watson", b"London", b"which", b"the "], buf
    buf.fill_(0x61)
    return [b"a", b"aa", b"aaa"], buf


def build(pats, **variants):
    b = ac.AhoCorasick.builder().kind(ac.AhoCorasickKind.DFA).gpu_engine("hot")
    for k, v in variants.items():
        b.gpu_variant(k, v)
    return b.build(pats)


def alternate(fns, steps=None):
    """fns: {label: callable returning ms}; warm-up, then the labels in turn, args.steps rounds -> {label: [ms]}"""
    for f in fns.values():
        f()
    ms = {k: [] for k in fns}
    for _ in range(steps or args.steps):
        for k, f in fns.items():
            ms[k].append(f())
    return ms


def report(inp, what, ms, size, **extra):
    row = {"input": inp, "compare": what, "bytes": size}
    for k, v in ms.items():
        row[k + "_ms"] = round(float(np.median(v)), 4)
        row[k + "_min_ms"] = round(min(v), 4)
    a, b = list(ms)[:2]
    row["ratio_%s_over_%s" % (a, b)] = round(float(np.median(ms[a]) / np.median(ms[b])), 3)
    row.update(extra)
    print(json.dumps(row), flush=True)


def wall(f):
    def g():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    return g


for inp in args.inputs.split(","):
    pats, buf = inputs(inp)
    hist, rec, noagree, walk = build(pats), build(pats, count_hist=0), build(pats, count_hist=2), build(pats, lw_events=0)
    out = torch.zeros(len(pats), dtype=torch.int64, device="cuda")
    prof = _lib.CProfile()
    # equal results at the timed size, every form
    want = hist.count_patterns(buf, out=out, profile=prof).cpu().numpy().copy()
    total = int(prof.n_matches)
    for a in (rec, noagree):
        assert np.array_equal(a.count_patterns(buf, out=out).cpu().numpy(), want), inp
    m, _ = walk.overlapping_device(buf, out=None, profile=prof)
    assert m == total == int(want.sum()) and prof.engine_used == 3, (inp, m, total)
    extra = {"patterns": len(pats), "matches": total, "bytes_per_match": round(n / max(total, 1), 1)}

    def scan_ms(a, count):
        def f():
            if count:
                a.count_patterns(buf, out=out, profile=prof)
            else:
                a.overlapping_device(buf, out=None, profile=prof)
            return float(prof.ms_scan)
        return f
    report(inp, "walk", alternate({"k_lw_hist": scan_ms(hist, True), "k_lw_count": scan_ms(walk, False)}), n, **extra)
    report(inp, "forms", alternate({"visits": wall(lambda: hist.count_patterns(buf, out=out)),
                                    "records": wall(lambda: rec.count_patterns(buf, out=out))}), n, **extra)
    if inp == "same":
        report(inp, "agree", alternate({"agree": scan_ms(hist, True), "per_lane": scan_ms(noagree, True)}), n, **extra)
    if inp != "sparse":
        small = buf if inp == "prose" else buf[: args.old_way_mib << 20]
        auto = ac.AhoCorasick.builder().kind(ac.AhoCorasickKind.DFA).build(pats)   # the parent's way: its own engine choice
        old = lambda: np.bincount(auto.find_overlapping_iter(small, as_numpy=True)["pattern"], minlength=len(pats))
        assert np.array_equal(old().astype(np.int64), hist.count_patterns(small).astype(np.int64)), inp
        report(inp, "old-way", alternate({"count_patterns": wall(lambda: hist.count_patterns(small)), "iter_bincount": wall(old)}, steps=3),
               int(small.numel()), **extra)
    del buf

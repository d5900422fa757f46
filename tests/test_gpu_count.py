"""Per-pattern occurrence counts (acgpu_count_patterns / AhoCorasick.count_patterns): the state-visit form on the LDS walk
(device/lds_hist.hip: k_lw_hist + k_hist_expand, every table flavour and class form) and the records form (k_hist_records
behind the overlapping search) against np.bincount of the oracle's ordered overlapping stream.  Integers: equality."""
import ctypes as C

import numpy as np
import pytest
import torch

import aho_corasick_amd as ac
from aho_corasick_amd import _lib
from gpu_util import build_pair
from oracle import orc

gpu = pytest.mark.gpu
N = (200 << 10) + 37   # seven 32 KiB wave regions: first and last on the edge walk, the middle ones interior
VISITS, RECORDS = 1, 0


def az(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(0x61, 0x7B, size=int(rng.integers(lo, hi + 1)), dtype=np.uint8)) for _ in range(n)]


def small_set():   # nested and duplicated 1-4 byte patterns over {a,b,c}: one pattern in the lists of several states
    rng = np.random.default_rng(31)
    return [bytes(rng.choice(np.frombuffer(b"abc", dtype=np.uint8), size=int(rng.integers(1, 5)))) for _ in range(14)] + [b"a", b"a"]


# name -> (patterns, alphabet (lo, span) of the haystack, build kind, variants, expected form)
CASES = {
    "full": (small_set, (0x61, 4), "dfa", {}, VISITS),
    "full-cls-lds": (small_set, (0x61, 4), "dfa", {"lw_cls": 0}, VISITS),
    "full-cls-computed": (small_set, (0x61, 4), "dfa", {"lw_cls": 1}, VISITS),
    "narrow": (lambda: orc.gen_patterns(1000, seed=0xAC01), (0x20, 95), "dfa", {}, VISITS),
    "narrow-cls-lds": (lambda: orc.gen_patterns(1000, seed=0xAC01), (0x20, 95), "dfa", {"lw_cls": 0}, VISITS),
    "narrow-cls-computed": (lambda: orc.gen_patterns(1000, seed=0xAC01), (0x20, 95), "dfa", {"lw_cls": 1}, VISITS),
    "wide": (lambda: orc.gen_patterns(1000, seed=0xAC01, lo=0x61, span=26), (0x61, 26), "dfa", {"lw_flavour": 1}, VISITS),
    "records-by-variant": (small_set, (0x61, 4), "dfa", {"count_hist": 0}, RECORDS),
    "records-empty-pattern": (lambda: small_set() + [b""], (0x61, 4), "dfa", {}, RECORDS),
    "records-large-set": (lambda: az(20000, 5, 12, 7), (0x61, 26), None, {}, RECORDS),
    "records-split-set": (lambda: az(1200, 9, 12, 9) + [b"ab", b"ca", b"b"], (0x61, 26), None, {}, RECORDS),
}


def bincount(stream, n, lo=None, hi=None):
    if lo is not None:   # a shard strictly inside the span: ends in (lo, hi]
        stream = stream[(stream["end"] > lo) & (stream["end"] <= hi)]
    return np.bincount(stream["pattern"].astype(np.int64), minlength=n).astype(np.uint64)


@gpu
@pytest.mark.parametrize("case", list(CASES))
def test_forms_and_automata(case):
    make, (lo, span), kind, variants, form = CASES[case]
    pats = make()
    a, o = build_pair(pats, "standard", {"kind": kind}, variants=variants)
    n = len(pats)
    hay = orc.gen_haystack(0, N, seed=0xAC02, lo=lo, span=span)
    for i, pos in enumerate(range(3, N, 997)):   # occurrences of the longer patterns too, across every region seam
        p = np.frombuffer(pats[(i * 7) % n], dtype=np.uint8)
        hay[pos:pos + len(p)] = p[: N - pos]
    dev = torch.from_numpy(hay).cuda()
    plan = (C.c_uint32 * 1)()
    assert ac.load_test_hooks().acgpu_test_count_plan(a._h, None, plan) == 0 and plan[0] == form

    def check(tensor, host, span=None, shard=None, ctx=""):
        inp, want = ac.Input(tensor), o.find_overlapping_iter(host, span=span, as_numpy=True)
        if span:
            inp.range(*span)
        prof = _lib.CProfile()
        got = a.count_patterns(inp, shard=shard, profile=prof)
        ref = bincount(want, n, *(shard or ()))
        assert got.dtype == np.uint64 and np.array_equal(got, ref), (case, ctx, np.nonzero(got != ref)[0][:5])
        assert prof.n_matches == int(ref.sum()), (case, ctx)
        return int(ref.sum())

    assert check(dev, hay, ctx="whole") > 200
    for off in (1, 5, 17):   # a tensor slice: the haystack pointer misaligned
        check(dev[off:], hay[off:], ctx=f"slice {off}")
    sub = (1003, N - 77)   # off the 16 / 64 / 128-byte grids at both ends
    check(dev, hay, span=sub, ctx="sub-span")
    assert check(dev, hay, span=sub, shard=(sub[0] + 4099, N - 12345), ctx="inner shard") > 100
    for k in (0, 1, 63):   # the empty span, edge walk only
        check(dev[:k], hay[:k], ctx=f"length {k}")


@gpu
@pytest.mark.parametrize("count_hist", [1, 2, 0])   # state visits with / without the wave-agreement shortcut, records
def test_hot_bin(count_hist):
    a, _ = build_pair([b"a", b"aa", b"aaa"], "standard", {"kind": "dfa"}, variants={"count_hist": count_hist})
    n = 300_000
    got = a.count_patterns(torch.full((n,), 0x61, dtype=torch.uint8, device="cuda"))
    assert got.tolist() == [n, n - 1, n - 2]


@gpu
def test_accumulate_and_zeroing():
    pats = small_set()
    a, o = build_pair(pats, "standard", {"kind": "dfa"})
    hays = [orc.gen_haystack(0, 50_001, seed=s, lo=0x61, span=4) for s in (1, 2)]
    refs = [bincount(o.find_overlapping_iter(h, as_numpy=True), len(pats)) for h in hays]
    out = torch.full((len(pats),), 12345, dtype=torch.int64, device="cuda")
    out.zero_()
    for h in hays:
        assert a.count_patterns(torch.from_numpy(h).cuda(), out=out, accumulate=True) is out
    assert np.array_equal(out.cpu().numpy().astype(np.uint64), refs[0] + refs[1])
    a.count_patterns(torch.from_numpy(hays[1]).cuda(), out=out)   # without the flag the call zeroes first
    assert np.array_equal(out.cpu().numpy().astype(np.uint64), refs[1])


@gpu
@pytest.mark.parametrize("count_hist", [1, 0])
def test_host_haystack(count_hist):
    a, _ = build_pair(small_set(), "standard", {"kind": "dfa"}, variants={"count_hist": count_hist})
    hay = orc.gen_haystack(0, 70_003, seed=3, lo=0x61, span=4)
    want = a.count_patterns(torch.from_numpy(hay).cuda())
    assert want.sum() > 1000
    assert np.array_equal(a.count_patterns(hay), want) and np.array_equal(a.count_patterns(hay.tobytes()), want)


def test_errors_are_decided_on_the_host():
    L = ac.load_library()
    a = ac.AhoCorasick.new([b"foo", b"bar"])
    ci, _keep = a._cinput(ac.Input(b"foobar"))
    buf = (C.c_uint64 * 3)()
    assert L.acgpu_count_patterns(a._h, C.byref(ci), 0, 6, buf, 3, 0, None, None) == 22   # ACGPU_ERR_INVALID_ARGUMENT
    assert b"n_counts" in L.acgpu_last_error()
    with pytest.raises(RuntimeError, match="ACGPU_COUNT_ACCUMULATE"):
        a.count_patterns(b"foobar", accumulate=True)   # host output
    with pytest.raises(ac.MatchError) as e:
        a.count_patterns(ac.Input(b"foobar").anchored(ac.Anchored.Yes))
    assert e.value.kind == "InvalidInputAnchored"
    with pytest.raises(ac.MatchError) as e:
        ac.AhoCorasick.builder().match_kind(ac.MatchKind.LeftmostFirst).build([b"foo"]).count_patterns(b"foo")
    assert e.value.kind == "UnsupportedOverlapping"

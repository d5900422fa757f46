"""-m gpu: the two-type prefix filter's deferred level-1 survivors (csrc/device/pf_scan.hip: PfWave::defer / drain_deferred) --
hit lanes queue one entry per row in LDS and are verified in dense batches of 64; a row pair whose hit lanes do not fit is
peeled in the row path.  Ordered records against the oracle's overlapping stream, with the engine requested by name: a scan
that abandoned itself and was repeated by another engine would show as engine_used != 4 or routed != 0.

A row is 1 008 bytes (63 lanes x 16), a task 40 rows = 40 320 bytes; the queue is empty at every task seam and holds 92 entries.

The probe (k_pf_probe) shares the wavefront code: test_probe_decisions_and_start_counts.  Its device counter is not
reported by any call, so the start count there is the host model's (acgpu_test_pf_host) over the probe's own samples."""
import ctypes as C

import numpy as np
import pytest
import torch

import aho_corasick_amd as ac
import corpora
from gpu_util import assert_same
from oracle import orc

pytestmark = pytest.mark.gpu

ROW, TASK = 1008, 40 * 1008
# 4-byte patterns of bytes the generated sets do not start with often: planted back to back they put several survivor
# bits into one lane
EXTRA = [b"Qz~j", b"w#K|", b"^y{V", b"}G`x"]


def build(pats, casei=False, variants=None):
    b = ac.AhoCorasick.builder().kind(ac.AhoCorasickKind.DFA).gpu_engine("pf").gpu_deterministic_routing(True) \
        .ascii_case_insensitive(casei)
    for k, v in (variants or {}).items():
        b.gpu_variant(k, v)
    return b.build(pats), orc.Oracle(pats, kind=orc.KIND_DFA, ascii_case_insensitive=casei)


@pytest.fixture(scope="module")
def headline():
    pats = orc.gen_patterns(1000, seed=0xAC01) + EXTRA
    return (pats,) + build(pats)


def check(a, o, hay, label, span=None, shard=None):
    d = torch.from_numpy(hay).cuda()
    want = o.find_overlapping_iter(hay, span=span, as_numpy=True)
    inp = ac.Input(d)
    if span is not None:
        inp.range(*span)
    prof = ac._lib.CProfile()
    if shard is None:
        got = a.find_overlapping_iter(inp, as_numpy=True, profile=prof)
    else:
        want = want[(want["end"] > shard[0]) & (want["end"] <= shard[1])]
        got = a.find_overlapping_shard(inp, shard[0], shard[1], profile=prof)
    assert int(prof.engine_used) == 4 and int(prof.routed) == 0, (label, int(prof.engine_used), int(prof.routed))
    assert_same(got, want, label)
    # the count-only call on the same input
    prof = ac._lib.CProfile()
    n, ok = a.overlapping_device(d, span=span, shard=shard, out=None, profile=prof)
    assert n == len(want) and int(prof.engine_used) == 4, (label, n, len(want))
    return want


def sparse(n, pats, seed, every=4099):
    """random printable text with whole patterns every `every` bytes, at the very start and flush with the end"""
    hay = orc.gen_haystack(0, n, seed=seed).copy()
    for k, at in enumerate(list(range(7, n, every)) + [0]):
        p = np.frombuffer(pats[(k * 7) % len(pats)], dtype=np.uint8)
        if at + len(p) <= n:
            hay[at:at + len(p)] = p
    p = np.frombuffer(pats[3], dtype=np.uint8)
    if len(p) <= n:
        hay[n - len(p):] = p
    return hay


LENGTHS = [1, 15, 16, 17, ROW - 1, ROW, ROW + 1, 2 * ROW, 2 * ROW + 1, TASK - 1, TASK, TASK + 1, 3 * TASK + 5, (300 << 10) + 777]


def test_lengths_across_the_seams(headline):
    pats, a, o = headline
    total = 0
    for n in LENGTHS:
        total += len(check(a, o, sparse(n, pats, 0xD0 + n % 251, every=509), f"length {n}"))
    assert total > 1000


def test_spans_and_shards_off_the_grid(headline):
    pats, a, o = headline
    n = 6 * TASK + 321
    hay = sparse(n, pats, 0xD1, every=211)
    for s0, s1 in ((1, n), (TASK + 1013, 3 * TASK - 777), (5, 2 * ROW + 9), (3 * TASK - 1, 3 * TASK + ROW + 1), (2 * TASK + 16 * 62 + 15, n - 3)):
        assert len(check(a, o, hay, f"span ({s0},{s1})", span=(s0, s1))) > 0
    for (s0, s1), (b0, b1) in (((0, n), (TASK + 5, 4 * TASK + 1)), ((33, n - 7), (2 * TASK - 3, 2 * TASK + ROW + 500)), ((0, n), (5 * TASK + 7, n))):
        assert len(check(a, o, hay, f"span ({s0},{s1}) shard ({b0},{b1})", span=(s0, s1), shard=(b0, b1))) > 0


def test_sparse_headline_input(headline):
    """the benchmark's input in small: the queue fills over ~8 row pairs, most tasks end on a partial batch"""
    pats, a, o = headline
    want = check(a, o, sparse((1 << 20) + 13, pats, 0xAC02, every=65521), "sparse")
    assert 10 < len(want) < 200


def test_several_survivor_bits_per_lane(headline):
    """4-byte patterns back to back at offsets 1, 5, 9, 13 and 0, 4, 8, 12 of a lane (every probe of the lane survives, in
    both rows of a pair), single ones at offsets 1 and 15, in lanes 0 and 62 and across the row wrap"""
    pats, a, o = headline
    n = 3 * TASK
    hay = orc.gen_haystack(0, n, seed=0xD2).copy()
    quad = np.frombuffer(b"".join(EXTRA), dtype=np.uint8)
    planted = 0
    for pair0 in (0, 6 * ROW, TASK - 2 * ROW, TASK, 2 * TASK + 18 * ROW):
        for row in (0, 1):
            base = pair0 + row * ROW
            for lane, off in ((1, 1 - row), (5, row), (31, 1 - row), (62, 1 - row)):
                at = base + 16 * lane + off
                hay[at:at + 16] = quad
                planted += 4
            for lane, off in ((0, 1), (0, 5), (9, 1), (9, 15), (17, 15), (40, 14), (50, 15)):
                at = base + 16 * lane + off
                hay[at:at + 4] = quad[:4]
                planted += 1
    for at in (2 * ROW + 16 * 62 + 15, 3 * ROW + 16 * 62 + 15, TASK + 5 * ROW + 16 * 62 + 15):   # lane 62 into the next row
        hay[at:at + 4] = quad[4:8]
        planted += 1
    want = check(a, o, hay, "multi-bit masks")
    assert len(want) >= planted


def dense_stretch(pats, n, seed):
    """4-byte pattern prefixes and whole patterns, concatenated: nearly every probe survives level 1"""
    rng = np.random.default_rng(seed)
    parts, have = [], 0
    while have < n:
        p = pats[int(rng.integers(len(pats)))]
        p = p if rng.integers(4) == 0 else p[:4]
        parts.append(p)
        have += len(p)
    return np.frombuffer(b"".join(parts), dtype=np.uint8)[:n]


def test_hit_dense_stretches(headline):
    """the queue overflows: row pairs peeled in the row path alternate with batches, and with queued sparse pairs around them"""
    pats, a, o = headline
    hay = orc.gen_haystack(0, 8 * TASK + 99, seed=0xD3).copy()
    for at, n in ((TASK + 333, 2 * TASK + 500), (5 * TASK - 7000, 3000), (7 * TASK, 3 * ROW)):
        hay[at:at + n] = dense_stretch(pats, n, at)
    assert len(check(a, o, hay, "dense stretches")) > 2000
    small = dense_stretch(pats, 30000, 5).copy()     # dense throughout, fewer than 1 024 starts per wavefront
    assert len(check(a, o, small, "dense throughout")) > 500


def test_case_folded_instance():
    pats = orc.gen_patterns(1000, seed=0xAC01)
    a, o = build(pats, casei=True)
    hay = orc.gen_haystack(0, 4 * TASK + 7, seed=0xD4).copy()
    for k, at in enumerate(range(11, len(hay) - 40, 1499)):
        p = pats[k % len(pats)]
        q = np.frombuffer(p.swapcase() if k % 2 else p.upper(), dtype=np.uint8)
        hay[at:at + len(q)] = q
    hay[2 * TASK:2 * TASK + 3000] = np.frombuffer(bytes(dense_stretch(pats, 3000, 9)).swapcase(), dtype=np.uint8)
    assert len(check(a, o, hay, "case-insensitive")) > 100


def test_exact_second_table_instance():
    """more than 24 000 patterns kept on this kernel (variant pfx_min_patterns): the second table keyed by true starts, whose
    64 KiB leave no room for the queue -- survivors are peeled in the row path"""
    pats = orc.gen_patterns(25000, seed=0xAC05)
    a, o = build(pats, variants={"pfx_min_patterns": 1 << 30})
    hay = sparse(3 * TASK + 5, pats, 0xD5, every=307)
    assert len(check(a, o, hay, "exact second table")) > 300


def test_chunk_counter_form(headline):
    """variant pf_classic: the scan credits chunk counters (no event list), a fill kernel writes the records"""
    pats, _, o = headline
    a, _ = build(pats, variants={"pf_classic": 1})
    hay = sparse(5 * TASK + 1, pats, 0xD6, every=401)
    hay[TASK:TASK + 5000] = dense_stretch(pats, 5000, 3)
    assert len(check(a, o, hay, "chunk counters")) > 500


def test_repeated_calls_leave_no_state(headline):
    pats, a, o = headline
    hays = [sparse(n, pats, 0xE0 + k, every=257) for k, n in enumerate((2 * TASK + 3, 37, 6 * TASK, ROW + 1, 3 * TASK - 1))]
    hays[2][TASK:3 * TASK] = dense_stretch(pats, 2 * TASK, 11)
    wants = [o.find_overlapping_iter(h, as_numpy=True) for h in hays]
    devs = [torch.from_numpy(h).cuda() for h in hays]
    for rnd in range(3):
        for k in (0, 1, 2, 3, 4, 2, 0):
            prof = ac._lib.CProfile()
            got = a.find_overlapping_iter(devs[k], as_numpy=True, profile=prof)
            assert int(prof.engine_used) == 4 and int(prof.routed) == 0
            assert_same(got, wants[k], f"round {rnd}, haystack {k}")


# level-2 hits of the host model over the probe's 256 samples of 8 064 bytes (each hands two starts to level 3), for the two
# inputs of the test below: with the parent commit's 64 KiB second table, and with the 32 KiB one
PROBE_L2_PARENT = {"dense": 159405, "sparse": 693}
PROBE_L2 = {"dense": 159467, "sparse": 1030}
# (routed, engine_used) of the calls below on the parent commit
PROBE_PARENT_CALLS = {"dense, first call": (1, 4), "dense, probed": (1, 4), "sparse, probed": (0, 4)}


def probe_samples_l2(a, hay):
    """the host model's level-2 hits over the samples launch_pf_probe takes of a whole-haystack search"""
    L = ac.load_test_hooks()
    L.acgpu_test_pf_host.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    stride = (len(hay) // 256) & ~15
    total = 0
    for k in range(256):
        piece = np.ascontiguousarray(hay[k * stride:k * stride + 8 * ROW])
        n, info = C.c_uint64(), (C.c_uint64 * 8)()
        assert L.acgpu_test_pf_host(a._h, C.c_void_p(piece.ctypes.data), len(piece), 0, C.byref(n), info) == 0 and int(info[0]) == 1
        total += int(info[3])
    return total


def test_probe_decisions_and_start_counts():
    """words-5000 with adaptive routing (the automaton's alternative is the large-set filter: the rule abandons the two-type
    filter from 0.06 starts per byte on).  Dense input = sherlock.txt: the first call's scan abandons itself, the second call
    asks the probe, which chooses the alternative.  Sparse input = random printable text on the same automaton: the probe
    keeps the filter.  The (routed, engine_used) pairs are those of the parent commit, from a run of this test's calls
    against a build of that commit on the same device; the start counts are the host model's over the probe's samples --
    PROBE_L2_PARENT from the parent commit's test hooks, PROBE_L2 from this tree's.  The 32 KiB table is the 64 KiB one with
    its halves or-ed together (the hash is masked), so it passes everything the parent's passed and a little more: on dense
    input +0.04 %, on sparse input +49 %, both on the same side of the rule as before."""
    ws = corpora.words("words-5000")
    a = ac.AhoCorasick.builder().build(ws)
    o = orc.Oracle(ws, kind=orc.KIND_CNFA)
    n = 32 << 20
    hays = {"dense": corpora.haystack("sherlock.txt", n), "sparse": orc.gen_haystack(0, n, seed=0xAC02)}
    for name, hay in hays.items():
        l2 = probe_samples_l2(a, hay)
        print(f"probe samples, {name}: level-2 hits {l2} (parent {PROBE_L2_PARENT[name]})")
        assert l2 == PROBE_L2[name] and l2 >= PROBE_L2_PARENT[name]
        # the routing rule on these counts (launch_pf_probe: 5000 X > route_cb B, route_cb = 300) lands where the device does
        for count in (l2, PROBE_L2_PARENT[name]):
            assert (5000 * 2 * count > 300 * 256 * 8 * ROW) == (name == "dense")
    prof = ac._lib.CProfile()
    seen = {}
    want = {k: o.find_overlapping_parallel(h)[0] for k, h in hays.items()}
    devs = {k: torch.from_numpy(h).cuda() for k, h in hays.items()}
    for label, k in (("dense, first call", "dense"), ("dense, probed", "dense"), ("sparse, probed", "sparse")):
        got = a.find_overlapping_iter(devs[k], as_numpy=True, profile=prof)
        assert_same(got, want[k], label)
        seen[label] = (int(prof.routed), int(prof.engine_used))
    print("probe calls (routed, engine_used):", seen)
    assert seen == PROBE_PARENT_CALLS

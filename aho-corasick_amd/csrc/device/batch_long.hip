// Long segments of the batched find for gfx950 (acgpu_find_batch, capi_batch.cpp): the segments the classify kernel of
// batch_find.hip lists instead of giving them to a lane -- a lane walks one byte per dependent LDS round trip, so a segment
// of megabytes on one lane would hold the whole call.  Such a segment [b, e) does not need a serial walk.  It needs ONE
// position p* from which the lane loop of k_batch_find, run on [p*, e) in the automaton's own tables, reports the segment's
// answer and ends within L = max_pattern_len bytes (DESIGN.md 3.2d "Long segments" has the arguments):
//   anchored search, or a set with an empty pattern      p* = b                    (no scout)
//   Standard rule (Standard automaton, or `earliest`)    p* = max(b, e_min - L)    e_min: smallest END of an occurrence in [b, e)
//   LeftmostFirst / LeftmostLongest                      p* = s_min                s_min: smallest START of an occurrence
// e_min and s_min are minima over the occurrences of the STANDARD automaton of the same patterns (the automaton itself, or
// its twin), and a minimum is order-free: it is taken chunk-parallel with every lane busy and combined by one 64-bit
// atomicMin per window into lkey[i], the key of entry i of the long list (UINT64_MAX: no occurrence).
//
// k_batch_scout.  Work unit: window w of a long segment owns the match ENDS in (b + w W, min(e, b + (w+1) W)]; lane l of the
// wave that takes it owns the ends of chunk l of C = W / 64 bytes.  The wave streams the window and L - 1 bytes of warm-up
// through its wave-private LDS tile with k_batch_find's loader (16-byte loads over the aligned hull, BatchArgs::mis for
// misaligned bases, ACGPU_HAY_CHECK on every load); LDS is laid out as there -- four tiles, the class map, the rows image
// when plan_batch gives the Standard automaton one -- so W = kBatchTile less the hull of the warm-up (batch_long_window).
// A lane starts at max(b, chunk begin - (L - 1)) in the unanchored start state and ignores match states at positions <=
// its chunk begin: an occurrence that ends at q starts at >= q - L, so the warm-up sees all of it.  At a match state at q
// the candidate is q (Standard rule) or q - len(first entry of the state's match list): that entry is the state's longest
// pattern -- host/builder.cpp puts a state's own pattern first (`owns`, step 3) and appends the list of its failure state,
// whose patterns are proper suffixes, behind it -- so it is the smallest start among the occurrences that end at q.  No
// list is read beyond first(), no record is formed.  A lane stops at its first candidate (Standard rule) or once an end
// can no longer start before its minimum s, i.e. behind s + L - 1 (leftmost rule).  Before loading a window the wave reads
// the segment's key and skips the window when no end in it can improve the key; the read races with the other waves on
// purpose: the key only decreases, so a stale value only costs work -- as long as the whole wave decides on ONE value (the
// first lane's), since the lanes load the tile together.  A call whose offsets the classify kernel refused serves no entry.
// Scheduling: persistent workgroups of four waves; the windows of all long segments are numbered consecutively, a
// segment's windows ascending, and a wave takes ids grid-stride, so early windows run first and the skips bite.  The id is
// mapped to (entry, window) by binary search in the prefix sum of the entries' window counts (k_batch_long_scan: their
// number is known on the device only).  One 100 MiB segment spreads over every compute unit as 100 000 segments of 40 KiB do.
//
// k_batch_resolve.  One lane per long entry: p* from the key, then try_find's loop (lane_begin / lane_match of
// batch_step.hpp; k_batch_find keeps its own copy of the same statements, see there) on [p*, e) with the call's anchored / earliest flags, on the global tables of
// the automaton itself, bytes straight from global memory; the 24-byte record goes to out[seg], the found counter to ctl[2].
#include <hip/hip_runtime.h>

#include <algorithm>

#include "batch_long.hpp"
#include "batch_step.hpp"
#include "host/engine_plan.hpp"
#include "launch_util.hpp"
#include "tile_walk.hpp"

namespace acgpu {

namespace {

using namespace batchdev;

constexpr uint32_t kBlTile = kBatchTile, kBlWaves = kBatchWaves, kBlBlock = kBatchWaves * 64;
constexpr uint32_t kBlClsOff = kBlWaves * kBlTile, kBlRowsOff = kBlClsOff + 256;   // (k_batch_find's layout)
constexpr uint32_t kBlScanBlock = 1024, kBlResolveBlock = 256;

// the first lane's value in every lane, and known to the compiler as uniform
__device__ __forceinline__ uint64_t wave_first_u64(uint64_t v) {
    return (uint64_t(uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(v >> 32))))) << 32) |
           uint32_t(__builtin_amdgcn_readfirstlane(int(uint32_t(v))));
}

// the entries of the long list to serve: none when the classify kernel found a bad offset -- the host refuses the call after
// the synchronisation, and the well-formed entries beside a bad one may add up to many times the haystack
__device__ __forceinline__ uint64_t n_long_of(const BatchArgs& a) {
    if (a.ctl[0] != ~0ull) return 0;
    const uint64_t n = a.ctl[1];
    return n < a.longs_cap ? n : a.longs_cap;
}

__global__ __launch_bounds__(kBlScanBlock) void k_batch_long_scan(BatchArgs a, BatchLongArgs la) {
    __shared__ uint64_t wsum[kBlScanBlock / 64];
    const uint64_t n_long = n_long_of(a);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint64_t base = 0; base < n_long; base += kBlScanBlock) {
        const uint64_t i = base + threadIdx.x;
        uint64_t v = 0;
        if (i < n_long) {
            const BatchLong g = a.longs[i];
            v = (g.end - g.begin + la.window - 1) / la.window;
        }
        uint64_t x = v;   // inclusive scan of the wave
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t t = __shfl_up(x, o, 64);
            if (int(lane) >= o) x += t;
        }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        uint64_t before = 0, all = 0;
        for (uint32_t w = 0; w < kBlScanBlock / 64; w++) {
            if (w < wave) before += wsum[w];
            all += wsum[w];
        }
        if (i < n_long) la.wpre[i] = carry + before + x - v;
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) la.wpre[n_long] = carry;
}

template <class S>
__global__ __launch_bounds__(kBlBlock) void k_batch_scout(S st, BatchArgs a, BatchLongArgs la) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint64_t n_long = n_long_of(a);
    if (n_long == 0) return;
    const uint64_t total = la.wpre[n_long];
    if (uint64_t(blockIdx.x) * kBlWaves >= total) return;   // (the whole workgroup: before the image is copied)
    // LDS: [kBlWaves tiles][class map][rows of the image]
    smem[kBlClsOff + threadIdx.x] = st.classes()[threadIdx.x];
    {
        const uint4* src = reinterpret_cast<const uint4*>(st.image());
        uint4* dst = reinterpret_cast<uint4*>(smem + kBlRowsOff);
        for (uint32_t i = threadIdx.x; i < st.image_bytes() / 16; i += kBlBlock) dst[i] = src[i];
    }
    __syncthreads();
    st.bind(smem + kBlRowsOff, smem + kBlClsOff);

    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint8_t* tile = smem + wave * kBlTile;
    const uint64_t W = la.window, C = la.window / 64, L = la.max_len;
    const bool leftmost = la.leftmost != 0;

    for (uint64_t id = uint64_t(blockIdx.x) * kBlWaves + wave; id < total; id += uint64_t(gridDim.x) * kBlWaves) {
        uint64_t lo = 0, hi = n_long;   // wpre[lo] <= id < wpre[hi]
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (la.wpre[mid] <= id) lo = mid; else hi = mid;
        }
        const BatchLong g = a.longs[lo];
        const uint64_t vb = g.begin + a.mis, ve = g.end + a.mis;   // virtual: v % 16 == 0 <=> a 16-byte aligned address
        const uint64_t wb = vb + (id - la.wpre[lo]) * W;
        if (wb >= ve) continue;
        const uint64_t we = ve - wb < W ? ve : wb + W;
        // one value for the whole wave: the lanes load a tile together, so they must skip or stay together, and nothing
        // promises that 64 lanes racing with another wave's atomicMin read the same word
        const uint64_t key = wave_first_u64(__atomic_load_n(&a.lkey[lo], __ATOMIC_RELAXED));
        const uint64_t kv = key == ~0ull ? key : key + a.mis;
        // the last end that can still improve the key
        uint64_t cap = leftmost ? (kv == ~0ull ? kv : kv + L - 1) : kv - 1;
        if (cap <= wb) continue;   // no end of this window can

        const uint64_t ws = wb - vb >= L - 1 ? wb - (L - 1) : vb;
        const uint64_t tb = ws & ~uint64_t(15);
        uint64_t lim = (we + 15) & ~uint64_t(15);
        if (lim > tb + kBlTile) lim = tb + kBlTile;   // (never: batch_long_window leaves room for the hull of the warm-up)
        wave_lds_fence();
        for (uint64_t v = tb + uint64_t(lane) * 16; v < lim; v += 64 * 16) {
            ACGPU_HAY_CHECK(a, v, 16);
            *reinterpret_cast<uint4*>(tile + (v - tb)) = *reinterpret_cast<const uint4*>(a.hay16 + v);
        }
        wave_lds_fence();

        const uint64_t cb = wb + lane * C;   // this lane owns the ends in (cb, ce]
        uint64_t ce = we - cb < C ? we : cb + C;
        if (cb >= we) ce = cb;
        if (ce > cap) ce = cap;
        if (ce > lim) ce = lim;
        uint64_t best = kv;
        if (cb < ce) {
            const uint64_t pos = cb - vb >= L - 1 ? cb - (L - 1) : vb;
            uint32_t k = uint32_t(pos - tb), ke = uint32_t(ce - tb);
            const uint32_t kc = uint32_t(cb - tb);
            uint32_t sid = st.start(false);
            uint32_t w = *reinterpret_cast<const uint32_t*>(tile + (k & ~3u));
            while (k < ke) {
                sid = st.next(false, sid, uint8_t(w >> (8 * (k & 3))));
                k++;
                if (st.is_special(sid)) {
                    if (sid == kDevDead) break;
                    if (k > kc && st.is_match(sid)) {
                        if (!leftmost) { best = tb + k; break; }
                        uint32_t pid, plen;
                        st.first(sid, pid, plen);
                        const uint64_t s = tb + k - plen;
                        if (s < best) {
                            best = s;
                            const uint64_t stop = s + L - 1;   // an end behind it starts behind s
                            if (stop < tb + ke) ke = stop > tb ? uint32_t(stop - tb) : 0;
                        }
                    }
                }
                if ((k & 3) == 0 && k < ke) w = *reinterpret_cast<const uint32_t*>(tile + k);
            }
        }
        const uint64_t m = wave_min_u64(best);
        if (lane == 0 && m < kv) atomicMin(&a.lkey[lo], static_cast<unsigned long long>(m - a.mis));
    }
}

template <class S>
__global__ __launch_bounds__(kBlResolveBlock) void k_batch_resolve(S st, BatchArgs a, BatchLongArgs la) {
    const uint64_t n_long = n_long_of(a);
    const bool anchored = a.anchored != 0, earliest = a.earliest != 0;
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t i0 = uint64_t(blockIdx.x) * kBlResolveBlock + (threadIdx.x - lane); i0 < n_long;
         i0 += uint64_t(gridDim.x) * kBlResolveBlock) {
        const uint64_t i = i0 + lane;
        bool found = false;
        if (i < n_long) {
            const BatchLong g = a.longs[i];
            const uint64_t vb = g.begin + a.mis, ve = g.end + a.mis;
            uint64_t p = vb;
            bool walk = true;
            if (la.scouted) {
                const uint64_t key = a.lkey[i];
                if (key == ~0ull) walk = false;   // no occurrence in the segment
                else if (la.leftmost) p = key + a.mis;
                else p = key - g.begin >= la.max_len ? key + a.mis - la.max_len : vb;
            }
            uint32_t m_pid = ACGPU_NO_MATCH;
            uint64_t m_start = 0, m_end = 0;
            if (walk && p >= vb && p <= ve) {
                uint32_t sid = st.start(anchored);
                bool done = lane_begin(st, earliest, p, sid, found, m_pid, m_start, m_end);
                for (uint64_t pos = p; !done && pos < ve;) {
                    ACGPU_HAY_CHECK(a, pos, 1);
                    sid = st.next(anchored, sid, a.hay16[pos]);
                    pos++;
                    if (st.is_special(sid)) {
                        if (sid == kDevDead) break;
                        if (st.is_match(sid)) done = lane_match(st, anchored, earliest, vb, pos, sid, found, m_pid, m_start, m_end);
                    }
                }
            }
            uint64_t* r = reinterpret_cast<uint64_t*>(a.out + g.seg);
            r[0] = m_pid;   // (pattern, _pad = 0)
            r[1] = found ? m_start - a.mis : 0;
            r[2] = found ? m_end - a.mis : 0;
        }
        const uint64_t hits = __ballot(found);
        if (lane == 0 && hits) atomicAdd(&a.ctl[2], static_cast<unsigned long long>(__popcll(hits)));
    }
}

template <class S>
hipError_t launch_scout_form(const S& st, uint32_t image_bytes, const BatchArgs& a, const BatchLongArgs& la, uint64_t max_windows,
                             uint32_t blocks, hipStream_t s) {
    const void* fn = reinterpret_cast<const void*>(&k_batch_scout<S>);
    if (hipError_t e = ensure_dynamic_lds(fn, int(kBatchLdsBytes)); e != hipSuccess) return e;
    const uint32_t lds = kBlRowsOff + image_bytes;
    if (lds > kBatchLdsBytes) return hipErrorInvalidValue;
    uint64_t resident = uint64_t(device_cus()) * std::min<uint32_t>(4u, kBatchLdsBytes / lds);
    if (blocks) resident = blocks;
    const uint64_t grid = std::min<uint64_t>((max_windows + kBlWaves - 1) / kBlWaves, resident);
    if (grid == 0) return hipSuccess;
    k_batch_scout<S><<<dim3(uint32_t(grid)), dim3(kBlBlock), lds, s>>>(st, a, la);
    return hipGetLastError();
}

template <class S>
hipError_t launch_resolve_form(const S& st, const BatchArgs& a, const BatchLongArgs& la, uint64_t max_long, hipStream_t s) {
    const uint64_t grid = std::min<uint64_t>((max_long + kBlResolveBlock - 1) / kBlResolveBlock, 1024);
    if (grid == 0) return hipSuccess;
    k_batch_resolve<S><<<dim3(uint32_t(grid)), dim3(kBlResolveBlock), 0, s>>>(st, a, la);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_batch_long_scan(const BatchArgs& a, const BatchLongArgs& la, hipStream_t s) {
    if (!la.wpre || la.window < 64) return hipErrorInvalidValue;
    k_batch_long_scan<<<dim3(1), dim3(kBlScanBlock), 0, s>>>(a, la);
    return hipGetLastError();
}

hipError_t launch_batch_scout(uint32_t form, const DevAutomaton& da, const BatchRows& rows, const BatchArgs& a, const BatchLongArgs& la,
                              uint64_t max_windows, uint32_t blocks, hipStream_t s) {
    if (!a.lkey || !la.wpre || la.max_len == 0 || la.window < 64 * 64 || la.window % 64 ||
        ((la.max_len - 1 + 30) & ~15u) + la.window > kBlTile)
        return hipErrorInvalidValue;
    if (form == uint32_t(BatchForm::LdsRows)) {
        if (!rows.rows || rows.rows_bytes % 16) return hipErrorInvalidValue;
        RowsStep st{rows, nullptr, nullptr};
        return launch_scout_form(st, rows.rows_bytes, a, la, max_windows, blocks, s);
    }
    if (form == uint32_t(BatchForm::DfaWalk) && da.has_dfa) {
        GlobalStep<DfaEng> st;
        st.eng.d = da.dfa; st.eng.cls = da.dfa.classes;
        return launch_scout_form(st, 0, a, la, max_windows, blocks, s);
    }
    if (form == uint32_t(BatchForm::CnfaWalk) && da.has_cnfa) {
        GlobalStep<CnfaEng> st;
        st.eng.c = da.cnfa; st.eng.cls = da.cnfa.classes;
        return launch_scout_form(st, 0, a, la, max_windows, blocks, s);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_batch_resolve(const DevAutomaton& da, const BatchArgs& a, const BatchLongArgs& la, uint64_t max_long, hipStream_t s) {
    if (la.scouted && !a.lkey) return hipErrorInvalidValue;
    if (da.has_dfa) {
        GlobalStep<DfaEng> st;
        st.eng.d = da.dfa; st.eng.cls = da.dfa.classes;
        return launch_resolve_form(st, a, la, max_long, s);
    }
    if (da.has_cnfa) {
        GlobalStep<CnfaEng> st;
        st.eng.c = da.cnfa; st.eng.cls = da.cnfa.classes;
        return launch_resolve_form(st, a, la, max_long, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace acgpu

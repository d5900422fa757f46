// Long segments of the batched OVERLAPPING iterator for gfx950 (acgpu_find_iter_batch, capi_batch_iter.cpp): the segments
// the classify kernel of batch_find.hip lists instead of giving them to a lane of k_batch_iter.  The overlapping iteration
// of a segment [b, e) is one walk whose state is never reset, and every match state emits its whole match list, so the
// records are a function of (end position, state) alone -- and the state at q is known from the L - 1 = max_pattern_len - 1
// bytes in front of q: a walk from the unanchored start state at p <= q - (L - 1) stands at q in the state of the walk from
// b (both are the longest suffix of the text that is a prefix of a pattern; it is at most L long, and a suffix of exactly L
// bytes is a whole pattern, which a state reached over >= L bytes holds as well).  So the walk is cut as the scout of
// batch_long.hip cuts it (DESIGN.md 3.2e "Long segments"):
//
// Work unit.  Window w of a long segment owns the match ENDS in (b + w W, min(e, b + (w + 1) W)], W = batch_long_window(L);
// lane l of the wave that takes it owns the ends of chunk l of C = W / 64 bytes, starts at max(b, chunk begin - (L - 1)) in
// the unanchored start state and ignores match states at positions <= its chunk begin.  Window 0, lane 0 also owns the end
// b itself: the match list of the start state (an empty pattern).  Records ordered by (window, lane, position, list order)
// are the records find_overlapping_iter gives on the span, in its order.  The windows of all long segments are numbered
// consecutively through wpre (k_batch_long_scan); persistent 4-wave workgroups take ids grid-stride and map an id to (entry,
// window) by binary search.  The wave streams the window and its warm-up through its wave-private tile with k_batch_find's
// loader (16-byte loads over the aligned hull, BatchArgs::mis for misaligned bases, ACGPU_HAY_CHECK on every load).  LDS is
// laid out as k_batch_iter has it -- four tiles, the class map, the staging areas of the fill pass, the rows image where
// plan_batch_iter grants it -- so the same automata walk in LDS here and there.
//
//   count   lane_cnt[id * 64 + l] = the lane's records (256 B per window), wsum[id] = the window's
//   prefix  one workgroup per long entry, looping over its windows: wsum[id] = the records of the segment's windows before
//           id; counts[seg] = the segment's records -- the call's ONE launch_scan then yields rec_off for short and long
//           segments together; a segment with 2^32 records or more sets control word [2], which the host reads with the others
//   fill    the same walk.  The window's records are out[rec_off[seg] + wsum[id] ...), a lane's part of them starts at the
//           exclusive prefix of the window's lane counts.  A window without a record is skipped before its tile is loaded, a
//           lane without one does not walk, and a lane stops at its last record.  Up to kBatchIterStage records are put
//           together in the wave's staging area and stored as 16-byte pieces (8-byte pieces at a misaligned head / tail);
//           larger ranges are stored by the lanes.  No lane stores outside its own part, whatever the walk finds.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "batch_iter_long.hpp"
#include "batch_step.hpp"
#include "host/engine_plan.hpp"
#include "launch_util.hpp"
#include "tile_walk.hpp"

namespace acgpu {

namespace {

using namespace batchdev;

constexpr uint32_t kIlTile = kBatchTile, kIlWaves = kBatchWaves, kIlBlock = kBatchWaves * 64;
constexpr uint32_t kIlClsOff = kIlWaves * kIlTile, kIlStageOff = kIlClsOff + 256;
constexpr uint32_t kIlStageWave = kBatchIterStage * sizeof(acgpu_match);
constexpr uint32_t kIlPrefixBlock = 256;
// LDS: [kIlWaves tiles][class map][fill: kIlWaves staging areas][rows of the image]   (k_batch_iter's layout)
template <bool FILL> constexpr uint32_t rows_off() { return kIlStageOff + (FILL ? kBatchIterStageBytes : 0u); }
static_assert(kIlStageWave * kIlWaves == kBatchIterStageBytes && kIlStageWave % 16 == 0, "staging as engine_plan.hpp budgets it");
static_assert(rows_off<true>() + 2 * kBatchIterRowsMaxEntries <= kBatchLdsBytes, "the largest image fits beside tiles and staging");

typedef __attribute__((address_space(3))) uint64_t lds_u64;

// the entries of the long list to serve: none when the classify kernel found a bad offset (the host refuses the call)
__device__ __forceinline__ uint64_t n_long_of(const BatchArgs& a) {
    if (a.ctl[0] != ~0ull) return 0;
    const uint64_t n = a.ctl[1];
    return n < a.longs_cap ? n : a.longs_cap;
}

__device__ __forceinline__ uint64_t wave_incl_scan_u64(uint64_t x, uint32_t lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t t = __shfl_up(x, o, 64);
        if (int(lane) >= o) x += t;
    }
    return x;
}

template <class S, bool FILL>
__global__ __launch_bounds__(kIlBlock) void k_batch_iter_long(S st, BatchIterArgs ia, BatchLongArgs la, BatchIterLongArgs ila) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const BatchArgs& a = ia.b;
    const uint64_t n_long = n_long_of(a);
    if (n_long == 0) return;
    uint64_t total = la.wpre[n_long];
    if (total > ila.cap_windows) total = ila.cap_windows;   // (never: the host sizes the arrays by an upper bound)
    if (uint64_t(blockIdx.x) * kIlWaves >= total) return;   // (the whole workgroup: before the image is copied)
    smem[kIlClsOff + threadIdx.x] = st.classes()[threadIdx.x];
    {
        const uint4* src = reinterpret_cast<const uint4*>(st.image());
        uint4* dst = reinterpret_cast<uint4*>(smem + rows_off<FILL>());
        for (uint32_t i = threadIdx.x; i < st.image_bytes() / 16; i += kIlBlock) dst[i] = src[i];
    }
    __syncthreads();
    st.bind(smem + rows_off<FILL>(), smem + kIlClsOff);

    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint8_t* tile = smem + wave * kIlTile;
    uint8_t* stage = smem + kIlStageOff + wave * kIlStageWave;   // (fill only)
    const uint64_t W = la.window, C = la.window / 64, warm = la.max_len ? la.max_len - 1 : 0;

    for (uint64_t id = uint64_t(blockIdx.x) * kIlWaves + wave; id < total; id += uint64_t(gridDim.x) * kIlWaves) {
        uint64_t lo = 0, hi = n_long;   // wpre[lo] <= id < wpre[hi]
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (la.wpre[mid] <= id) lo = mid; else hi = mid;
        }
        const BatchLong g = a.longs[lo];
        const uint64_t widx = id - la.wpre[lo];
        const uint64_t vb = g.begin + a.mis, ve = g.end + a.mis;   // virtual: v % 16 == 0 <=> a 16-byte aligned address
        const uint64_t wb = vb + widx * W;
        const bool live = wb < ve;   // (always: an entry has ceil(length / W) windows)
        const uint64_t we = !live ? wb : (ve - wb < W ? ve : wb + W);

        // fill: the window's range of records (wave-uniform) and this lane's part of it
        uint32_t quota = 0;
        uint64_t my_off = 0, wtot = 0, base = 0;
        if (FILL) {
            quota = ila.lane_cnt[id * 64 + lane];
            const uint64_t x = wave_incl_scan_u64(quota, lane);
            wtot = __shfl(x, 63, 64);
            if (wtot == 0 || !live) continue;
            my_off = x - quota;
            base = ia.rec_off[g.seg] + ila.wsum[id];
        }
        const bool staged = FILL && wtot <= kBatchIterStage;

        const uint64_t ws = wb - vb >= warm ? wb - warm : vb;
        const uint64_t tb = ws & ~uint64_t(15);
        uint64_t lim = (we + 15) & ~uint64_t(15);
        if (lim > tb + kIlTile) lim = tb + kIlTile;   // (never: batch_long_window leaves room for the hull of the warm-up)
        if (live) {
            wave_lds_fence();
            for (uint64_t v = tb + uint64_t(lane) * 16; v < lim; v += 64 * 16) {
                ACGPU_HAY_CHECK(a, v, 16);
                *reinterpret_cast<uint4*>(tile + (v - tb)) = *reinterpret_cast<const uint4*>(a.hay16 + v);
            }
            wave_lds_fence();
        }

        uint64_t n = 0;   // records of this lane so far
        bool done = !live || (FILL && quota == 0);
        auto emit = [&](uint32_t pid, uint64_t ms, uint64_t me) {
            if (FILL && n < quota) {   // (never outside this lane's part, whatever the walk finds)
                // (pattern, _pad = 0), start, end.  Two branches and an explicit LDS pointer: one pointer for both is a flat one
                if (staged) {
                    lds_u64* r = (lds_u64*)(stage + (my_off + n) * sizeof(acgpu_match));
                    r[0] = pid; r[1] = ms - a.mis; r[2] = me - a.mis;
                } else {
                    uint64_t* r = reinterpret_cast<uint64_t*>(a.out + base + my_off + n);
                    r[0] = pid; r[1] = ms - a.mis; r[2] = me - a.mis;
                }
            }
            n++;
            if (FILL && n >= quota) done = true;
        };
        // every pattern of the match state `sid`, in list order, ending at me
        auto emit_list = [&](uint32_t sid, uint64_t me) {
            const uint32_t len = st.list_len(sid);
            if (!FILL) { n += len; return; }
            for (uint32_t i = 0; i < len && !done; i++) {
                uint32_t pid, plen;
                st.list_at(sid, i, pid, plen);
                emit(pid, me - plen, me);
            }
        };

        if (!done && widx == 0 && lane == 0) {   // the end b itself: the start state's own list
            const uint32_t s0 = st.start(false);
            if (st.is_match(s0)) emit_list(s0, vb);
        }
        const uint64_t cb = wb + lane * C;   // this lane owns the ends in (cb, ce]
        uint64_t ce = cb >= we ? cb : (we - cb < C ? we : cb + C);
        if (ce > lim) ce = lim;
        if (!done && cb < ce) {
            const uint64_t pos = cb - vb >= warm ? cb - warm : vb;
            uint32_t k = uint32_t(pos - tb);
            const uint32_t ke = uint32_t(ce - tb), kc = uint32_t(cb - tb);
            uint32_t sid = st.start(false);
            uint32_t w = *reinterpret_cast<const uint32_t*>(tile + (k & ~3u));
            while (k < ke) {
                sid = st.next(false, sid, uint8_t(w >> (8 * (k & 3))));
                k++;
                if (st.is_special(sid)) {
                    if (sid == kDevDead) break;
                    if (k > kc && st.is_match(sid)) {
                        emit_list(sid, tb + k);
                        if (done) break;
                    }
                }
                if ((k & 3) == 0 && k < ke) w = *reinterpret_cast<const uint32_t*>(tile + k);
            }
        }

        if (!FILL) {
            ila.lane_cnt[id * 64 + lane] = uint32_t(n);   // (a count beyond 32 bits: the segment's sum refuses the call)
            const uint64_t x = wave_incl_scan_u64(n, lane);
            if (lane == 63) ila.wsum[id] = x;
            continue;
        }
        if (staged) {   // the window's records, put together in LDS, as one contiguous piece
            wave_lds_fence();
            const uint32_t nbytes = uint32_t(wtot) * uint32_t(sizeof(acgpu_match));
            uint8_t* dst = reinterpret_cast<uint8_t*>(a.out + base);
            const uint32_t head = (reinterpret_cast<uintptr_t>(dst) & 15) ? 8u : 0u;
            const uint32_t body_end = head + ((nbytes - head) & ~15u);
            if (head && lane == 0) *reinterpret_cast<uint64_t*>(dst) = *reinterpret_cast<const uint64_t*>(stage);
            for (uint32_t o = head + lane * 16; o < body_end; o += 64 * 16) {
                const uint2 x = *reinterpret_cast<const uint2*>(stage + o), y = *reinterpret_cast<const uint2*>(stage + o + 8);
                *reinterpret_cast<uint4*>(dst + o) = make_uint4(x.x, x.y, y.x, y.y);
            }
            if (body_end < nbytes && lane == 63) *reinterpret_cast<uint64_t*>(dst + body_end) = *reinterpret_cast<const uint64_t*>(stage + body_end);
            wave_lds_fence();
        }
    }
}

__global__ __launch_bounds__(kIlPrefixBlock) void k_batch_iter_long_prefix(BatchIterArgs ia, BatchLongArgs la, BatchIterLongArgs ila) {
    __shared__ uint64_t part[kIlPrefixBlock / 64];
    const BatchArgs& a = ia.b;
    const uint64_t n_long = n_long_of(a);
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint64_t i = blockIdx.x; i < n_long; i += gridDim.x) {
        uint64_t w0 = la.wpre[i], w1 = la.wpre[i + 1];
        if (w0 > ila.cap_windows) w0 = ila.cap_windows;
        if (w1 > ila.cap_windows) w1 = ila.cap_windows;
        uint64_t carry = 0;
        for (uint64_t at = w0; at < w1; at += kIlPrefixBlock) {
            const uint64_t id = at + threadIdx.x;
            const uint64_t v = id < w1 ? ila.wsum[id] : 0;
            const uint64_t x = wave_incl_scan_u64(v, lane);
            if (lane == 63) part[wave] = x;
            __syncthreads();
            uint64_t before = 0, all = 0;
            for (uint32_t w = 0; w < kIlPrefixBlock / 64; w++) {
                if (w < wave) before += part[w];
                all += part[w];
            }
            if (id < w1) ila.wsum[id] = carry + before + x - v;
            carry += all;
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            ia.counts[a.longs[i].seg] = uint32_t(carry);
            if (carry > 0xFFFFFFFFull) atomicOr(&a.ctl[2], 1ull);   // the host refuses the call
        }
    }
}

template <class S, bool FILL>
hipError_t launch_pass(const S& st, uint32_t image_bytes, const BatchIterArgs& a, const BatchLongArgs& la, const BatchIterLongArgs& ila,
                       uint32_t blocks, hipStream_t s) {
    const void* fn = reinterpret_cast<const void*>(&k_batch_iter_long<S, FILL>);
    if (hipError_t e = ensure_dynamic_lds(fn, int(kBatchLdsBytes)); e != hipSuccess) return e;
    const uint32_t lds = rows_off<FILL>() + image_bytes;
    if (lds > kBatchLdsBytes) return hipErrorInvalidValue;
    uint64_t resident = uint64_t(device_cus()) * std::min<uint32_t>(4u, kBatchLdsBytes / lds);
    if (blocks) resident = blocks;
    const uint64_t grid = std::min<uint64_t>((ila.cap_windows + kIlWaves - 1) / kIlWaves, resident);
    if (grid == 0) return hipSuccess;
    k_batch_iter_long<S, FILL><<<dim3(uint32_t(grid)), dim3(kIlBlock), lds, s>>>(st, a, la, ila);
    return hipGetLastError();
}

template <bool FILL>
hipError_t launch_form(uint32_t form, const DevAutomaton& da, const BatchIterRows& rows, const BatchIterArgs& a, const BatchLongArgs& la,
                       const BatchIterLongArgs& ila, uint32_t blocks, hipStream_t s) {
    const uint32_t warm = la.max_len ? la.max_len - 1 : 0;
    if (!la.wpre || !ila.lane_cnt || !ila.wsum || !a.overlapping || a.b.anchored || la.window < 64 * 64 || la.window % 64 ||
        ((warm + 30) & ~15u) + la.window > kIlTile)
        return hipErrorInvalidValue;
    if (form == uint32_t(BatchForm::LdsRows)) {
        if (!rows.r.rows || rows.r.rows_bytes % 16 || !rows.list_off || !rows.list) return hipErrorInvalidValue;
        RowsListStep st;
        st.t = rows.r; st.rows = nullptr; st.cls = nullptr; st.list_off = rows.list_off; st.list = rows.list;
        return launch_pass<RowsListStep, FILL>(st, rows.r.rows_bytes, a, la, ila, blocks, s);
    }
    if (form == uint32_t(BatchForm::DfaWalk) && da.has_dfa) {
        GlobalStep<DfaEng> st;
        st.eng.d = da.dfa; st.eng.cls = da.dfa.classes;
        return launch_pass<GlobalStep<DfaEng>, FILL>(st, 0, a, la, ila, blocks, s);
    }
    if (form == uint32_t(BatchForm::CnfaWalk) && da.has_cnfa) {
        GlobalStep<CnfaEng> st;
        st.eng.c = da.cnfa; st.eng.cls = da.cnfa.classes;
        return launch_pass<GlobalStep<CnfaEng>, FILL>(st, 0, a, la, ila, blocks, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_batch_iter_long_count(uint32_t form, const DevAutomaton& da, const BatchIterRows& rows, const BatchIterArgs& a,
                                        const BatchLongArgs& la, const BatchIterLongArgs& ila, uint32_t blocks, hipStream_t s) {
    return launch_form<false>(form, da, rows, a, la, ila, blocks, s);
}

hipError_t launch_batch_iter_long_prefix(const BatchIterArgs& a, const BatchLongArgs& la, const BatchIterLongArgs& ila, uint64_t max_long,
                                         hipStream_t s) {
    if (!la.wpre || !ila.wsum || !a.counts) return hipErrorInvalidValue;
    const uint64_t grid = std::min<uint64_t>(max_long, 1024);
    if (grid == 0) return hipSuccess;
    k_batch_iter_long_prefix<<<dim3(uint32_t(grid)), dim3(kIlPrefixBlock), 0, s>>>(a, la, ila);
    return hipGetLastError();
}

hipError_t launch_batch_iter_long_fill(uint32_t form, const DevAutomaton& da, const BatchIterRows& rows, const BatchIterArgs& a,
                                       const BatchLongArgs& la, const BatchIterLongArgs& ila, uint32_t blocks, hipStream_t s) {
    return launch_form<true>(form, da, rows, a, la, ila, blocks, s);
}

}  // namespace acgpu

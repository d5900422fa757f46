// Batched iterator for gfx950 (acgpu_find_iter_batch, capi_batch_iter.cpp): EVERY match of every segment of a packed
// haystack, each segment searched as the reference's find_iter (or find_overlapping_iter) searches
// Input::new(H).span(off[s]..off[s+1]).  Output is CSR: the records of segment s are out[rec_off[s] .. rec_off[s+1]).
//
// Work split and tile streaming are those of the batched find (batch_find.hip): a wave task is 64 consecutive segments, one
// per lane; persistent 4-wave workgroups take tasks from a grid-stride loop; the task's bytes are streamed through the
// wave-private tile with coalesced 16-byte loads over the aligned hull, and the tile's origin is the lowest position an
// unfinished lane stands at.
//
// Per-lane loop.  Non-overlapping: FindIter (src/automaton.rs:857-936) as k_find_iter_serial restates it -- a chain of
// try_find searches (the loop of dev_try_find_fwd), each from the start state at the end of the last match, with the
// caller's `earliest` kept and handle_overlapping_empty_match (:910-920) per lane.  A search ends in a dead state, at its
// first match under earliest semantics, or at the segment's end; the lane then emits the pending match and restarts at
// m.end.  For the leftmost kinds m.end lies BEHIND the lane's position (the walk went on looking for a longer match), by up
// to max_pattern_len bytes, and possibly in front of the tile's origin: the lane sets pos = m.end and leaves the inner loop,
// and the next wave minimum moves the tile back -- the loader knows nothing of it.
// Overlapping (Standard automata): one walk per segment, the state never reset; at every match state the whole match list
// is emitted in list order (try_find_overlapping_fwd, :1443-1534).
//
// Termination.  The end of the last emitted match grows with every emission: a search from S reports an end >= S, the next
// one starts there, and one that would report the same empty match again is repeated from S + 1 (the `+1` rule), so every
// restart begins strictly behind the previous one except after an empty match, which that rule advances.  Every search
// walks forward only and ends at the segment's end at the latest; the lane standing at the tile's origin always has bytes
// in the tile, so every round of the wave loop steps at least one lane or ends one search.
//
// Two passes over one template (Sink = count | fill, Overlapping = false | true):
//   count  every lane counts its segment's records into counts[s] (a long segment: 0; the host serves it)
//   scan   launch_scan (kernels.hip): counts -> rec_off[0..n) and the total; launch_batch_iter_seal stores rec_off[n]
//   fill   the same walk; a lane is finished as soon as it has emitted rec_off[s+1] - rec_off[s] records -- at once when that
//          is 0, so tiles of match-free segments are never loaded and tasks without records are skipped.  The task's records
//          are one contiguous range of `out`: up to kBatchIterStage of them are put together in a wave-private LDS area and
//          stored as 16-byte pieces (8-byte pieces at a misaligned head / tail); larger ranges are stored by the lanes.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "batch_iter.hpp"
#include "batch_step.hpp"
#include "host/engine_plan.hpp"
#include "launch_util.hpp"
#include "tile_walk.hpp"

namespace acgpu {

namespace {

using namespace batchdev;

constexpr uint32_t kBiTile = kBatchTile, kBiWaves = kBatchWaves, kBiBlock = kBatchWaves * 64;
constexpr uint32_t kBiClsOff = kBiWaves * kBiTile, kBiStageOff = kBiClsOff + 256;
constexpr uint32_t kBiStageWave = kBatchIterStage * sizeof(acgpu_match);
// LDS: [kBiWaves tiles][class map][fill: kBiWaves staging areas][rows of the image]
template <bool FILL> constexpr uint32_t rows_off() { return kBiStageOff + (FILL ? kBatchIterStageBytes : 0u); }
static_assert(kBiStageWave * kBiWaves == kBatchIterStageBytes && kBiStageWave % 16 == 0, "staging as engine_plan.hpp budgets it");
static_assert(rows_off<true>() + 2 * kBatchIterRowsMaxEntries <= kBatchLdsBytes, "the largest image fits beside tiles and staging");

typedef __attribute__((address_space(3))) uint64_t lds_u64;

template <class S, bool FILL, bool OVL>
__global__ __launch_bounds__(kBiBlock) void k_batch_iter(S st, BatchIterArgs ia) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const BatchArgs& a = ia.b;
    smem[kBiClsOff + threadIdx.x] = st.classes()[threadIdx.x];
    {
        const uint4* src = reinterpret_cast<const uint4*>(st.image());
        uint4* dst = reinterpret_cast<uint4*>(smem + rows_off<FILL>());
        for (uint32_t i = threadIdx.x; i < st.image_bytes() / 16; i += kBiBlock) dst[i] = src[i];
    }
    __syncthreads();
    st.bind(smem + rows_off<FILL>(), smem + kBiClsOff);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint8_t* tile = smem + wave * kBiTile;
    uint8_t* stage = smem + kBiStageOff + wave * kBiStageWave;   // (fill only)
    const bool anchored = a.anchored != 0, earliest = a.earliest != 0;
    const uint64_t n_tasks = (a.n_seg + 63) / 64;

    for (uint64_t task = uint64_t(blockIdx.x) * kBiWaves + wave; task < n_tasks; task += uint64_t(gridDim.x) * kBiWaves) {
        const uint64_t seg = task * 64 + lane;
        const bool valid = seg < a.n_seg;
        // the task's range of records (wave-uniform), this lane's part of it
        uint64_t task_lo = 0, task_hi = 0, my_off = 0;
        uint32_t quota = 0;
        if (FILL) {
            task_lo = ia.rec_off[task * 64];
            task_hi = ia.rec_off[task * 64 + 64 < a.n_seg ? task * 64 + 64 : a.n_seg];
            if (task_hi <= task_lo) continue;
            if (valid) {
                my_off = ia.rec_off[seg];
                const uint64_t nx = ia.rec_off[seg + 1];
                quota = nx > my_off ? uint32_t(nx - my_off) : 0u;
            }
        }
        const bool staged = FILL && task_hi - task_lo <= kBatchIterStage;
        uint64_t b = 0, e = 0;
        if (valid) { b = a.off[seg]; e = a.off[seg + 1]; }
        if (b > a.hay_len) b = a.hay_len;
        if (e > a.hay_len) e = a.hay_len;
        if (e < b) e = b;
        const uint64_t vb = b + a.mis, ve = e + a.mis;   // virtual: v % 16 == 0 <=> a 16-byte aligned address
        bool done = !valid || e - b > a.lane_max || (FILL && quota == 0);   // (a long segment: served by the host)
        uint32_t n_emit = 0;

        auto emit = [&](uint32_t pid, uint64_t ms, uint64_t me) {
            if (FILL && n_emit < quota) {   // (never outside this lane's part, whatever the walk finds)
                // (pattern, _pad = 0), start, end.  Two branches and an explicit LDS pointer: one pointer for both is a flat one
                if (staged) {
                    lds_u64* r = (lds_u64*)(stage + (my_off - task_lo + n_emit) * sizeof(acgpu_match));
                    r[0] = pid; r[1] = ms - a.mis; r[2] = me - a.mis;
                } else {
                    uint64_t* r = reinterpret_cast<uint64_t*>(a.out + my_off + n_emit);
                    r[0] = pid; r[1] = ms - a.mis; r[2] = me - a.mis;
                }
            }
            n_emit++;
            if (FILL && n_emit >= quota) done = true;
        };

        // ---- the search in progress: from the start state at `srch`, now at `pos` in state `sid`, best match so far m_*
        uint64_t pos = vb, srch = vb, m_start = 0, m_end = 0, last_end = 0;
        uint32_t sid = 0, m_pid = 0;
        bool found = false, has_last = false, retry = false;
        auto start_search = [&](uint64_t at) -> bool {   // true: it is over at once
            srch = pos = at;
            sid = st.start(anchored);
            found = false;
            if (st.is_match(sid)) {   // match at the start state (an empty pattern)
                uint32_t plen;
                st.first(sid, m_pid, plen);
                m_end = at; m_start = at - plen;
                found = true;
            }
            return (found && earliest) || pos >= ve;
        };
        auto settle = [&](bool over) {   // FindIter's step behind a finished search; leaves a search in progress, or done
            while (over && !done) {
                if (!found) { done = true; break; }
                if (m_start == m_end && has_last && m_end == last_end && !retry) {   // handle_overlapping_empty_match
                    retry = true;
                    if (srch + 1 > ve) { done = true; break; }
                    over = start_search(srch + 1);
                    continue;
                }
                emit(m_pid, m_start, m_end);
                has_last = true; last_end = m_end; retry = false;
                if (done) break;
                over = start_search(m_end);
            }
        };
        if (!done) {
            if (OVL) {
                sid = st.start(anchored);
                if (st.is_match(sid)) {
                    const uint32_t n = st.list_len(sid);
                    for (uint32_t i = 0; i < n && !done; i++) {
                        uint32_t pid, plen;
                        st.list_at(sid, i, pid, plen);
                        emit(pid, vb - plen, vb);
                    }
                }
                if (pos >= ve) done = true;
            } else {
                settle(start_search(vb));
            }
        }

        for (;;) {
            uint64_t tb = wave_min_u64(done ? ~0ull : pos);
            if (tb == ~0ull) break;   // every lane is finished
            tb &= ~uint64_t(15);
            const uint64_t top = (wave_max_u64(done ? 0ull : ve) + 15) & ~uint64_t(15);
            const uint64_t lim = tb + kBiTile < top ? tb + kBiTile : top;
            wave_lds_fence();
            for (uint64_t v = tb + uint64_t(lane) * 16; v < lim; v += 64 * 16) {
                ACGPU_HAY_CHECK(a, v, 16);
                *reinterpret_cast<uint4*>(tile + (v - tb)) = *reinterpret_cast<const uint4*>(a.hay16 + v);
            }
            wave_lds_fence();
            // (pos >= tb by the origin rule; a lane restarted behind the tile waits for the tile to come back)
            while (!done && pos >= tb && pos < tb + kBiTile) {
                uint32_t k = uint32_t(pos - tb);
                const uint32_t ke = uint32_t((ve < tb + kBiTile ? ve : tb + kBiTile) - tb);
                bool over = false;
                uint32_t w = *reinterpret_cast<const uint32_t*>(tile + (k & ~3u));
                while (k < ke) {
                    sid = st.next(anchored, sid, uint8_t(w >> (8 * (k & 3))));
                    k++;
                    if (st.is_special(sid)) {
                        if (sid == kDevDead) { over = true; break; }
                        if (st.is_match(sid)) {
                            const uint64_t me = tb + k;
                            if (OVL) {
                                const uint32_t n = st.list_len(sid);
                                for (uint32_t i = 0; i < n && !done; i++) {
                                    uint32_t pid, plen;
                                    st.list_at(sid, i, pid, plen);
                                    emit(pid, me - plen, me);
                                }
                                if (done) break;
                            } else {
                                uint32_t pid, plen;
                                st.first(sid, pid, plen);
                                const uint64_t ms = me - plen;
                                if (!(anchored && ms > srch)) {
                                    m_pid = pid; m_start = ms; m_end = me;
                                    found = true;
                                    if (earliest) { over = true; break; }
                                }
                            }
                        }
                    }
                    if ((k & 3) == 0 && k < ke) w = *reinterpret_cast<const uint32_t*>(tile + k);
                }
                pos = tb + k;
                if (pos >= ve) over = true;
                if (OVL) {
                    if (over) done = true;
                    break;
                }
                if (!over) break;   // the tile is used up
                settle(true);
            }
        }

        if (!FILL) {
            if (valid) ia.counts[seg] = n_emit;   // (the 64 counts of a task: one contiguous piece)
            continue;
        }
        if (staged) {   // the task's records, put together in LDS, as one contiguous piece
            wave_lds_fence();
            const uint32_t nbytes = uint32_t(task_hi - task_lo) * uint32_t(sizeof(acgpu_match));
            uint8_t* dst = reinterpret_cast<uint8_t*>(a.out + task_lo);
            const uint32_t head = (reinterpret_cast<uintptr_t>(dst) & 15) ? 8u : 0u;
            const uint32_t body_end = head + ((nbytes - head) & ~15u);
            if (head && lane == 0) *reinterpret_cast<uint64_t*>(dst) = *reinterpret_cast<const uint64_t*>(stage);
            for (uint32_t o = head + uint32_t(lane) * 16; o < body_end; o += 64 * 16) {
                const uint2 x = *reinterpret_cast<const uint2*>(stage + o), y = *reinterpret_cast<const uint2*>(stage + o + 8);
                *reinterpret_cast<uint4*>(dst + o) = make_uint4(x.x, x.y, y.x, y.y);
            }
            if (body_end < nbytes && lane == 63) *reinterpret_cast<uint64_t*>(dst + body_end) = *reinterpret_cast<const uint64_t*>(stage + body_end);
            wave_lds_fence();
        }
    }
}

__global__ void k_batch_iter_seal(const uint64_t* totals, uint64_t* rec_off_end) {
    if (threadIdx.x == 0) *rec_off_end = totals[0];
}

template <class S, bool FILL>
hipError_t launch_pass(const S& st, uint32_t image_bytes, const BatchIterArgs& a, uint32_t blocks, hipStream_t s) {
    const void* fn = a.overlapping ? reinterpret_cast<const void*>(&k_batch_iter<S, FILL, true>)
                                   : reinterpret_cast<const void*>(&k_batch_iter<S, FILL, false>);
    if (hipError_t e = ensure_dynamic_lds(fn, int(kBatchLdsBytes)); e != hipSuccess) return e;
    const uint32_t lds = rows_off<FILL>() + image_bytes;
    if (lds > kBatchLdsBytes) return hipErrorInvalidValue;
    const uint64_t need = ((a.b.n_seg + 63) / 64 + kBiWaves - 1) / kBiWaves;
    // persistent workgroups: as many as the device holds at this LDS footprint (up to four per compute unit)
    uint64_t resident = uint64_t(device_cus()) * std::min<uint32_t>(4u, kBatchLdsBytes / lds);
    if (blocks) resident = blocks;
    const uint64_t grid = std::min<uint64_t>(need, resident);
    if (grid == 0) return hipSuccess;
    if (a.overlapping) k_batch_iter<S, FILL, true><<<dim3(uint32_t(grid)), dim3(kBiBlock), lds, s>>>(st, a);
    else k_batch_iter<S, FILL, false><<<dim3(uint32_t(grid)), dim3(kBiBlock), lds, s>>>(st, a);
    return hipGetLastError();
}

template <bool FILL>
hipError_t launch_form(uint32_t form, const DevAutomaton& da, const BatchIterRows& rows, const BatchIterArgs& a, uint32_t blocks,
                       hipStream_t s) {
    if (form == uint32_t(BatchForm::LdsRows)) {
        if (!rows.r.rows || rows.r.rows_bytes % 16 || !rows.list_off || !rows.list) return hipErrorInvalidValue;
        RowsListStep st;
        st.t = rows.r; st.rows = nullptr; st.cls = nullptr; st.list_off = rows.list_off; st.list = rows.list;
        return launch_pass<RowsListStep, FILL>(st, rows.r.rows_bytes, a, blocks, s);
    }
    if (form == uint32_t(BatchForm::DfaWalk) && da.has_dfa) {
        GlobalStep<DfaEng> st;
        st.eng.d = da.dfa; st.eng.cls = da.dfa.classes;
        return launch_pass<GlobalStep<DfaEng>, FILL>(st, 0, a, blocks, s);
    }
    if (form == uint32_t(BatchForm::CnfaWalk) && da.has_cnfa) {
        GlobalStep<CnfaEng> st;
        st.eng.c = da.cnfa; st.eng.cls = da.cnfa.classes;
        return launch_pass<GlobalStep<CnfaEng>, FILL>(st, 0, a, blocks, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_batch_iter_count(uint32_t form, const DevAutomaton& da, const BatchIterRows& rows, const BatchIterArgs& a,
                                   uint32_t blocks, hipStream_t s) {
    return launch_form<false>(form, da, rows, a, blocks, s);
}

hipError_t launch_batch_iter_fill(uint32_t form, const DevAutomaton& da, const BatchIterRows& rows, const BatchIterArgs& a,
                                  uint32_t blocks, hipStream_t s) {
    return launch_form<true>(form, da, rows, a, blocks, s);
}

hipError_t launch_batch_iter_seal(const uint64_t* totals, uint64_t* rec_off_end, hipStream_t s) {
    k_batch_iter_seal<<<dim3(1), dim3(64), 0, s>>>(totals, rec_off_end);
    return hipGetLastError();
}

}  // namespace acgpu

// Batched find for gfx950 (acgpu_find_batch, capi_batch.cpp): the first match of EVERY segment of a packed haystack, each
// segment searched as the reference's try_find searches Input::new(H).span(off[s]..off[s+1]) -- the loop of
// dev_try_find_fwd (kernels.hip; src/automaton.rs:1285-1420), one segment per wavefront lane, from the automaton's own
// start state in its own tables: all three match kinds and anchored mode come out exact, nothing is selected afterwards.
//
// Work split.  A wave task is 64 consecutive segments; their bytes are one contiguous range of the haystack.  The wave
// streams that range through a wave-private LDS tile of kBatchTile bytes: 16-byte loads over the aligned hull, coalesced
// (lane l takes 16-byte part l, l + 64, ...), clamped to the hull of the bytes the lanes still need.  The tile's origin is
// the lowest position an unfinished lane stands at, so tiles nobody needs -- the inside of a segment that is too long for a
// lane, the rest of segments that already reported -- are never loaded, and the loop ends when every lane is finished
// (found under earliest semantics, dead, or at its segment end).  A lane walks the part of its segment that lies in the tile
// and carries state, found flag and best match to the next one.  Persistent workgroups take tasks from a grid-stride loop;
// nothing in the walk is bounded by anything but a segment's length and lane_max, and whatever the offsets hold the kernel
// reads only inside the haystack (positions are clamped, end < begin is an empty segment).
//
// Records.  The 64 records of a task are 1 536 contiguous bytes: they are put together in the wave's tile and stored as such.
//
// Steppers (one skeleton, a template parameter; batch_step.hpp): the LDS rows of host/batch_tables.hpp -- one class lookup
// and one ds_read_u16 per byte --, DfaEng and CnfaEng on the global tables; all read the segment bytes from the same tile.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "batch_find.hpp"
#include "batch_step.hpp"
#include "host/engine_plan.hpp"
#include "launch_util.hpp"
#include "tile_walk.hpp"

namespace acgpu {

namespace {

using namespace batchdev;   // the steppers: batch_step.hpp

constexpr uint32_t kBfTile = kBatchTile, kBfWaves = kBatchWaves, kBfBlock = kBatchWaves * 64;
constexpr uint32_t kBfClsOff = kBfWaves * kBfTile, kBfRowsOff = kBfClsOff + 256;
static_assert(kBfRowsOff + 2 * kBatchRowsMaxEntries <= kBatchLdsBytes, "the largest image fits beside the tiles");
static_assert(64 * sizeof(acgpu_match) <= kBfTile && kBfTile % 1024 == 0, "a task's records are staged in its tile");

__global__ void k_batch_init(unsigned long long* ctl) {
    if (threadIdx.x == 0) { ctl[0] = ~0ull; ctl[1] = 0; ctl[2] = 0; }
}

__global__ __launch_bounds__(256) void k_batch_classify(BatchArgs a) {
    for (uint64_t s = uint64_t(blockIdx.x) * 256 + threadIdx.x; s < a.n_seg; s += uint64_t(gridDim.x) * 256) {
        const uint64_t b = a.off[s], e = a.off[s + 1];
        if (e < b || e > a.hay_len) {
            atomicMin(&a.ctl[0], static_cast<unsigned long long>(s));
        } else if (e - b > a.lane_max) {
            const unsigned long long i = atomicAdd(&a.ctl[1], 1ull);
            if (i < a.longs_cap) {
                a.longs[i] = BatchLong{s, b, e};
                if (a.lkey) a.lkey[i] = ~0ull;   // (batch_long.hip: no occurrence seen)
            }
        }
    }
}

template <class S>
__global__ __launch_bounds__(kBfBlock) void k_batch_find(S st, BatchArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    // LDS: [kBfWaves tiles][class map][rows of the image]
    smem[kBfClsOff + threadIdx.x] = st.classes()[threadIdx.x];
    {
        const uint4* src = reinterpret_cast<const uint4*>(st.image());
        uint4* dst = reinterpret_cast<uint4*>(smem + kBfRowsOff);
        for (uint32_t i = threadIdx.x; i < st.image_bytes() / 16; i += kBfBlock) dst[i] = src[i];
    }
    __syncthreads();
    st.bind(smem + kBfRowsOff, smem + kBfClsOff);

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint8_t* tile = smem + wave * kBfTile;
    const bool anchored = a.anchored != 0, earliest = a.earliest != 0;
    const uint64_t n_tasks = (a.n_seg + 63) / 64;

    for (uint64_t task = uint64_t(blockIdx.x) * kBfWaves + wave; task < n_tasks; task += uint64_t(gridDim.x) * kBfWaves) {
        const uint64_t seg = task * 64 + lane;
        const bool valid = seg < a.n_seg;
        uint64_t b = 0, e = 0;
        if (valid) { b = a.off[seg]; e = a.off[seg + 1]; }
        if (b > a.hay_len) b = a.hay_len;
        if (e > a.hay_len) e = a.hay_len;
        if (e < b) e = b;
        const uint64_t vb = b + a.mis, ve = e + a.mis;   // virtual: v % 16 == 0 <=> a 16-byte aligned address
        bool done = !valid || e - b > a.lane_max;        // (a long segment: listed by the classify kernel, served by batch_long.hip or the host)
        bool found = false;
        uint32_t m_pid = ACGPU_NO_MATCH;
        uint64_t m_start = 0, m_end = 0;
        uint64_t pos = vb;
        uint32_t sid = 0;
        if (!done) {
            sid = st.start(anchored);
            if (st.is_match(sid)) {   // match at the start state (an empty pattern)
                uint32_t pid, plen;
                st.first(sid, pid, plen);
                m_pid = pid; m_end = vb; m_start = vb - plen;
                found = true;
                if (earliest) done = true;
            }
            if (pos == ve) done = true;
        }

        for (;;) {
            uint64_t tb = wave_min_u64(done ? ~0ull : pos);
            if (tb == ~0ull) break;   // every lane is finished
            tb &= ~uint64_t(15);
            const uint64_t top = (wave_max_u64(done ? 0ull : ve) + 15) & ~uint64_t(15);
            const uint64_t lim = tb + kBfTile < top ? tb + kBfTile : top;
            wave_lds_fence();
            for (uint64_t v = tb + uint64_t(lane) * 16; v < lim; v += 64 * 16) {
                ACGPU_HAY_CHECK(a, v, 16);
                *reinterpret_cast<uint4*>(tile + (v - tb)) = *reinterpret_cast<const uint4*>(a.hay16 + v);
            }
            wave_lds_fence();
            if (!done && pos < tb + kBfTile) {
                uint32_t k = uint32_t(pos - tb);
                const uint32_t ke = uint32_t((ve < tb + kBfTile ? ve : tb + kBfTile) - tb);
                uint32_t w = *reinterpret_cast<const uint32_t*>(tile + (k & ~3u));
                while (k < ke) {
                    sid = st.next(anchored, sid, uint8_t(w >> (8 * (k & 3))));
                    k++;
                    if (st.is_special(sid)) {
                        if (sid == kDevDead) { done = true; break; }
                        if (st.is_match(sid)) {
                            uint32_t pid, plen;
                            st.first(sid, pid, plen);
                            const uint64_t me = tb + k, ms = me - plen;
                            if (!(anchored && ms > vb)) {
                                m_pid = pid; m_start = ms; m_end = me;
                                found = true;
                                if (earliest) { done = true; break; }
                            }
                        }
                    }
                    if ((k & 3) == 0 && k < ke) w = *reinterpret_cast<const uint32_t*>(tile + k);
                }
                pos = tb + k;
                if (pos >= ve) done = true;
            }
        }

        // the task's records, staged in the tile and stored as one contiguous piece
        wave_lds_fence();
        {
            uint64_t* r = reinterpret_cast<uint64_t*>(tile + lane * sizeof(acgpu_match));
            r[0] = m_pid;   // (pattern, _pad = 0)
            r[1] = found ? m_start - a.mis : 0;
            r[2] = found ? m_end - a.mis : 0;
        }
        wave_lds_fence();
        const uint64_t n_here = a.n_seg - task * 64 < 64 ? a.n_seg - task * 64 : 64;
        const uint32_t nbytes = uint32_t(n_here * sizeof(acgpu_match));
        uint8_t* dst = reinterpret_cast<uint8_t*>(a.out) + task * (64 * sizeof(acgpu_match));
        if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
            for (uint32_t o = uint32_t(lane) * 16; o < nbytes; o += 64 * 16) {
                if (o + 16 <= nbytes) *reinterpret_cast<uint4*>(dst + o) = *reinterpret_cast<const uint4*>(tile + o);
                else *reinterpret_cast<uint64_t*>(dst + o) = *reinterpret_cast<const uint64_t*>(tile + o);
            }
        } else {
            for (uint32_t o = uint32_t(lane) * 8; o < nbytes; o += 64 * 8)
                *reinterpret_cast<uint64_t*>(dst + o) = *reinterpret_cast<const uint64_t*>(tile + o);
        }
        const uint64_t hits = __ballot(found && valid);
        if (lane == 0 && hits) atomicAdd(&a.ctl[2], static_cast<unsigned long long>(__popcll(hits)));
    }
}

template <class S>
hipError_t launch_form(const S& st, uint32_t image_bytes, const BatchArgs& a, uint32_t blocks, hipStream_t s) {
    const void* fn = reinterpret_cast<const void*>(&k_batch_find<S>);
    if (hipError_t e = ensure_dynamic_lds(fn, int(kBatchLdsBytes)); e != hipSuccess) return e;
    const uint32_t lds = kBfRowsOff + image_bytes;
    if (lds > kBatchLdsBytes) return hipErrorInvalidValue;
    const uint64_t need = ((a.n_seg + 63) / 64 + kBfWaves - 1) / kBfWaves;
    // persistent workgroups: as many as the device holds at this LDS footprint (up to four per compute unit)
    uint64_t resident = uint64_t(device_cus()) * std::min<uint32_t>(4u, kBatchLdsBytes / lds);
    if (blocks) resident = blocks;
    const uint64_t grid = std::min<uint64_t>(need, resident);
    if (grid == 0) return hipSuccess;
    k_batch_find<S><<<dim3(uint32_t(grid)), dim3(kBfBlock), lds, s>>>(st, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_batch_classify(const BatchArgs& a, hipStream_t s) {
    k_batch_init<<<dim3(1), dim3(64), 0, s>>>(a.ctl);
    const uint64_t blocks = std::min<uint64_t>((a.n_seg + 255) / 256, 1024);
    if (blocks) k_batch_classify<<<dim3(uint32_t(blocks)), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_batch_find(uint32_t form, const DevAutomaton& da, const BatchRows& rows, const BatchArgs& a, uint32_t blocks,
                             hipStream_t s) {
    if (form == uint32_t(BatchForm::LdsRows)) {
        if (!rows.rows || rows.rows_bytes % 16) return hipErrorInvalidValue;
        RowsStep st{rows, nullptr, nullptr};
        return launch_form(st, rows.rows_bytes, a, blocks, s);
    }
    if (form == uint32_t(BatchForm::DfaWalk) && da.has_dfa) {
        GlobalStep<DfaEng> st;
        st.eng.d = da.dfa; st.eng.cls = da.dfa.classes;
        return launch_form(st, 0, a, blocks, s);
    }
    if (form == uint32_t(BatchForm::CnfaWalk) && da.has_cnfa) {
        GlobalStep<CnfaEng> st;
        st.eng.c = da.cnfa; st.eng.cls = da.cnfa.classes;
        return launch_form(st, 0, a, blocks, s);
    }
    return hipErrorInvalidValue;
}

}  // namespace acgpu

// Per-pattern occurrence counts (acgpu_count_patterns, capi_count.cpp) for gfx950: how often every pattern occurred, with no
// match record written anywhere.
//
// State-visit form (k_lw_hist + k_hist_expand).  The LDS transition walk of lds_walk.hip -- same image, same three table
// flavours and class forms, same persistent 1 024-thread workgroups, same register double-buffering of the haystack --
// counts how often every MATCH STATE is entered by an owned byte instead of adding up match-list lengths:
//     visits[s] += 1        for the state s behind every owned matching byte
// and the match lists are consulted once per call, not once per occurrence:
//     counts[p] = sum over the match states s whose list holds p of visits[s]                     (k_hist_expand)
// The walk's dependent chain never reads a list: a state with 4 095 patterns costs one add per visit.
//   * The bins are u32 words in LDS behind the image (16-byte aligned) whenever image + 4 * match states fit the budget:
//     zeroed beside the image copy, bumped by LDS atomics, flushed at the workgroup's end (non-zero bins only) by 64-bit
//     global atomics into visits[].  Otherwise every bump is a 64-bit global atomic on visits[] itself.
//   * A u32 bin cannot overflow: a bin gains at most one visit per byte its workgroup walks (+ 1 for the start state), and
//     launch_lw_hist puts the bins into LDS only when the bytes one workgroup can be handed -- ceil(tasks / waves) tasks
//     per wavefront, 16 wavefronts, 64 lane-chunks each -- stay below 2^32; beyond that (spans of a TiB) it takes the
//     global bins.  The bound comes from the span and the grid; nothing is flushed in between.
//   * Hot bins: on input where every lane of a wavefront enters the same state at the same step (one repeated byte),
//     same-address LDS atomics serialise.  With `agree` the flagged lanes first compare their bin with the first flagged
//     lane's (readlane + ballot): if all agree ONE lane adds the population count.  A/B: profiles/count_hist_ab.txt.
//
// Records form (k_hist_records): every automaton the LDS walk does not serve -- the overlapping search leaves its ordered
// records in scratch and one thread per record bumps counts[pattern], runs of one pattern within a wavefront combined into one
// add (the stream is ordered by end: runs are the norm on dense input).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../host/lw_tables.hpp"
#include "hot.hpp"
#include "launch_util.hpp"
#include "lw_dev.hpp"

namespace acgpu {

namespace {

using namespace lwdev;

constexpr int kLhBlock = 1024;
constexpr int kLhWaves = kLhBlock / 64;

struct LwHistArgs {
    unsigned long long* visits;   // [n_bins], zero on entry
    uint32_t n_bins;              // match states
    uint32_t bins_off;            // LDS byte offset of the u32 bins (behind the image, 16-byte aligned); 0: bins in visits[] only
    uint32_t agree;               // wave-agreement shortcut of the flagged path
    uint32_t full_recip;          // kLwFull: ceil(2^32 / row_bytes) -- row address -> row index by one v_mul_hi
    uint32_t first_match;         // kLwFull: bin = hid - first_match, hid = row index + 1
};

struct LwBins {
    uint32_t* lds;                // nullptr: global bins
    unsigned long long* glob;
    uint32_t n_bins, agree;
    int lane;
    __device__ __forceinline__ void add(uint32_t bin, uint32_t n) const {
        if (bin >= n_bins) return;   // (table invariant; the walk's fast path never depends on it)
        if (lds) (void)__hip_atomic_fetch_add(lds + bin, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else (void)__hip_atomic_fetch_add(glob + bin, static_cast<unsigned long long>(n), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // one visit of `bin` for every lane with `pred`; called by all lanes of the branch (ballots inside)
    __device__ __forceinline__ void add_if(uint32_t bin, bool pred) const {
        if (agree) {
            const uint64_t m = __ballot(pred);
            if (m == 0) return;
            const int first = __ffsll(static_cast<long long>(m)) - 1;
            const uint32_t b0 = uint32_t(__builtin_amdgcn_readlane(int(bin), first));
            if (__ballot(pred && bin == b0) == m) {
                if (lane == first) add(b0, uint32_t(__popcll(m)));
                return;
            }
        }
        if (pred) add(bin, 1);
    }
};

// bin of the state behind an EXACT handle, or ~0 when it is no match state (virtual slots resolved as in lw_match_len)
template <int FLAV>
__device__ __forceinline__ uint32_t lh_bin(const LwArgs& a, const LwHistArgs& x, const LwLds& L, uint32_t h) {
    if constexpr (FLAV == kLwFull) {
        if ((h & kLwFullLenMask) == 0) return ~0u;
        return __umulhi(h >> 16, x.full_recip) + 1 - x.first_match;
    }
    uint32_t da = h & 0xFFFFu;
    if (da >= a.virt_addr) da = 4 * L.rd16(a.vhid_off + ((da - a.virt_addr) >> 1));   // first slot of a multi state
    return da >= a.fm_addr ? (da - a.fm_addr) >> 2 : ~0u;
}

// One dword = 4 fast steps (lw_step4 of lw_dev.hpp) whose owned matching bytes bump bins.
template <int FLAV, bool CC, bool OWNED>
__device__ __forceinline__ void lh_step4(const LwArgs& a, const LwHistArgs& x, const LwLds& L, const LwCc& cc, const LwBins& B, uint32_t w,
                                         uint32_t& h) {
    constexpr bool X4 = FLAV == kLwFull;
    const uint32_t cv0 = lw_clsval<CC, 0, X4>(L, cc, w), cv1 = lw_clsval<CC, 1, X4>(L, cc, w);
    const uint32_t cv2 = lw_clsval<CC, 2, X4>(L, cc, w), cv3 = lw_clsval<CC, 3, X4>(L, cc, w);
    if constexpr (FLAV == kLwFull) {
        const uint32_t h1 = L.rd32(lw_addr_full(h, cv0));
        const uint32_t h2 = L.rd32(lw_addr_full(h1, cv1));
        const uint32_t h3 = L.rd32(lw_addr_full(h2, cv2));
        const uint32_t h4 = L.rd32(lw_addr_full(h3, cv3));
        h = h4;
        if (OWNED) {
            // the count the walk forms anyway: four match-list lengths of at most 4 095 in the low half of the sum
            const bool flag = ((h1 + h2 + h3 + h4) & kLwFullSumMask) != 0;
            if (__builtin_expect(__any(flag), 0)) {
                B.add_if(lh_bin<FLAV>(a, x, L, h1), flag && (h1 & kLwFullLenMask));
                B.add_if(lh_bin<FLAV>(a, x, L, h2), flag && (h2 & kLwFullLenMask));
                B.add_if(lh_bin<FLAV>(a, x, L, h3), flag && (h3 & kLwFullLenMask));
                B.add_if(lh_bin<FLAV>(a, x, L, h4), flag && (h4 & kLwFullLenMask));
            }
        }
    } else {
        const uint32_t rb = a.row_bytes;
        auto addr = [&](uint32_t hh, uint32_t c) { return FLAV == kLwWide ? lw_addr_wide(hh, c, rb) : lw_addr(hh, c, rb); };
        const uint32_t h0 = h;
        const uint32_t h1 = L.rd32(addr(h0, cv0));
        const uint32_t h2 = L.rd32(addr(h1, cv1));
        const uint32_t h3 = L.rd32(addr(h2, cv2));
        const uint32_t h4 = L.rd32(addr(h3, cv3));
        h = h4;
        const uint32_t worst = lw_max3_u16(lw_max3_u16(h1, h2, h3), h4, h4) & 0xFFFFu;
        const bool flag = worst >= a.fm_addr;
        if (__builtin_expect(__any(flag), 0)) {
            const bool redo = flag && worst >= a.virt_addr;   // a multi state or poison: the handles are not exact
            if (redo) {
                uint32_t hh = h0;
#pragma unroll 1
                for (int k = 0; k < 4; k++) {
                    hh = lw_careful_step<FLAV, CC>(a, L, hh, (w >> (8 * k)) & 0xFFu);
                    if (OWNED) B.add(lh_bin<FLAV>(a, x, L, hh), 1);
                }
                h = hh;
            }
            if (OWNED) {   // match states only: exact handles, bin = (da - fm_addr) / 4
                const bool exact = flag && !redo;
                const uint32_t d1 = h1 & 0xFFFFu, d2 = h2 & 0xFFFFu, d3 = h3 & 0xFFFFu, d4 = h4 & 0xFFFFu;
                B.add_if((d1 - a.fm_addr) >> 2, exact && d1 >= a.fm_addr);
                B.add_if((d2 - a.fm_addr) >> 2, exact && d2 >= a.fm_addr);
                B.add_if((d3 - a.fm_addr) >> 2, exact && d3 >= a.fm_addr);
                B.add_if((d4 - a.fm_addr) >> 2, exact && d4 >= a.fm_addr);
            }
        }
    }
}

// k_lw_count's skeleton (lds_walk.hip): what differs is what an owned matching byte does.
template <int UP, int FLAV, bool CC>
__global__ __launch_bounds__(kLhBlock) void k_lw_hist(LwArgs a, ScanGeom g, LwHistArgs x) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kLwLdsBytes];   // static, at LDS address 0: no base add per lookup
    uint32_t* const lds_bins = x.bins_off ? reinterpret_cast<uint32_t*>(lds + x.bins_off) : nullptr;
    {
        const uint4* src = reinterpret_cast<const uint4*>(a.image);
        uint4* dst = reinterpret_cast<uint4*>(lds);
        for (uint32_t i = threadIdx.x; i < a.image_bytes / 16; i += kLhBlock) dst[i] = src[i];
        if (lds_bins) for (uint32_t i = threadIdx.x; i < x.n_bins; i += kLhBlock) lds_bins[i] = 0;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t wave_id = uint64_t(blockIdx.x) * kLhWaves + wave;
    const uint64_t n_waves = uint64_t(gridDim.x) * kLhWaves;
    const uint32_t C = a.lane_chunk;
    const uint32_t warm_bytes = a.warm_pieces * 16;
    const uint32_t n_main = C / 16;   // pieces of an owned lane-chunk (multiple of 4)
    const LwLds L{lds};
    const LwBins B{lds_bins, x.visits, x.n_bins, x.agree, lane};
    LwCc cc;
    cc.add = uint32_t(a.cc_add); cc.hi = uint32_t(a.cc_hi);
    asm volatile("v_mov_b32 %0, %1" : "=v"(cc.v_lo) : "s"(a.cc_lo));   // opaque: the compiler must keep it in a VGPR

    const uint64_t region_bytes = uint64_t(64) * C;
    auto is_interior = [&](uint64_t lo) {
        return lo >= g.emit_lo && lo + region_bytes <= g.emit_hi && lo >= g.cold_floor + warm_bytes;
    };
    uint4 ua[UP], ub[UP];
    bool have_ua = false;   // ua holds unit 0 of this task: the previous task of the wave loaded it under its last unit
    for (uint64_t task = wave_id; task < a.n_tasks; task += n_waves) {
        const uint64_t j0 = task * 64;                           // first lane-chunk of the wave
        const uint64_t region_lo = g.grid0 + j0 * C;
        const bool interior = is_interior(region_lo);
        const uint64_t next_lo = region_lo + n_waves * region_bytes;
        const bool next_interior = task + n_waves < a.n_tasks && is_interior(next_lo);
        if (interior) {
            const uint8_t* p_main = g.hay16 + region_lo + uint64_t(lane) * C;
            uint32_t h = a.start;
            auto ld = [&](const uint8_t* p) {
                ACGPU_HAY_CHECK(g, uint64_t(p - g.hay16), 16);
                return *reinterpret_cast<const uint4*>(p);
            };
            // 128-byte units double-buffered in registers, every line requested once (see k_lw_count)
            auto ld_unit_at = [&](uint4 (&u)[UP], const uint8_t* p) __attribute__((always_inline)) {
#pragma unroll
                for (int k = 0; k < UP; k++) u[k] = ld(p + 16 * k);
            };
            auto piece = [&](const uint4& q, auto owned) __attribute__((always_inline)) {
                constexpr bool OW = decltype(owned)::value;
                lh_step4<FLAV, CC, OW>(a, x, L, cc, B, q.x, h);
                lh_step4<FLAV, CC, OW>(a, x, L, cc, B, q.y, h);
                lh_step4<FLAV, CC, OW>(a, x, L, cc, B, q.z, h);
                lh_step4<FLAV, CC, OW>(a, x, L, cc, B, q.w, h);
            };
            auto do_unit = [&](const uint4 (&u)[UP]) __attribute__((always_inline)) {
#pragma unroll
                for (int k = 0; k < UP; k++) piece(u[k], std::true_type{});
            };
            const uint32_t n_units = n_main / UP;
            // warm-up pieces (walked first, un-owned) and unit 0 in flight together
            {
                uint4 wq = make_uint4(0, 0, 0, 0);
                if (a.warm_pieces) wq = ld(p_main - 16 * a.warm_pieces);
                if (!have_ua) ld_unit_at(ua, p_main);
                for (uint32_t wp = a.warm_pieces; wp > 0; wp--) {
                    piece(wq, std::false_type{});
                    if (wp > 1) wq = ld(p_main - 16 * (wp - 1));
                }
            }
#pragma unroll 1
            for (uint32_t u0 = 0; u0 < n_units; u0 += 2) {
                // unconditional prefetches (a conditional load would put s_waitcnt vmcnt(0) in front of every use); behind the
                // last unit of the chunk the prefetch fetches unit 0 of the wave's next task
                ld_unit_at(ub, p_main + (16 * UP) * (u0 + 1 < n_units ? u0 + 1 : n_units - 1));
                do_unit(ua);
                {
                    const bool more = u0 + 2 < n_units;
                    const uint8_t* pn = more ? p_main + (16 * UP) * (u0 + 2)
                                             : next_interior ? g.hay16 + next_lo + uint64_t(lane) * C
                                                             : p_main + (16 * UP) * (n_units - 1);
                    ld_unit_at(ua, pn);
                }
                if (u0 + 1 < n_units) do_unit(ub);
            }
            have_ua = next_interior;
        } else {
            have_ua = false;
            const uint64_t j = j0 + uint64_t(lane);
            if (j < a.n_lane_chunks) {
                const uint64_t glo = g.grid0 + j * C, ghi = glo + C;
                const uint64_t lo = glo > g.emit_lo ? glo : g.emit_lo;
                const uint64_t hi = ghi < g.emit_hi ? ghi : g.emit_hi;
                if (j == 0 && g.emit_start_matches) B.add(lh_bin<FLAV>(a, x, L, a.start), 1);   // empty patterns at span_start
                if (hi > lo) {
                    uint64_t w = lo >= g.halo ? lo - g.halo : 0;
                    if (w < g.cold_floor) w = g.cold_floor;
                    lw_edge_walk_each<FLAV, CC>(a, L, g, w, lo, hi, [&](uint32_t hh) { B.add(lh_bin<FLAV>(a, x, L, hh), 1); });
                }
            }
        }
    }
    if (lds_bins) {   // flush: the non-zero bins of this workgroup
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < x.n_bins; i += kLhBlock) {
            const uint32_t v = lds_bins[i];
            if (v) (void)__hip_atomic_fetch_add(x.visits + i, static_cast<unsigned long long>(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// ---- expansion: counts[p] += visits[s] for every p in the list of s.  WAVE: one wavefront per match state (long lists),
// else one thread per match state.  The atomic is needed: a pattern sits in the list of every state it is a suffix of.
constexpr int kHxBlock = 256;
template <bool WAVE>
__global__ __launch_bounds__(kHxBlock) void k_hist_expand(const unsigned long long* __restrict__ visits, const uint32_t* __restrict__ moff,
                                                          const uint32_t* __restrict__ mpid, uint32_t n_states,
                                                          unsigned long long* __restrict__ counts, unsigned long long* __restrict__ total) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t t = uint64_t(blockIdx.x) * kHxBlock + threadIdx.x;
    const uint64_t s = WAVE ? t >> 6 : t;
    unsigned long long mine = 0;   // occurrences this thread accounts for
    if (s < n_states) {
        const unsigned long long v = visits[s];
        if (v) {
            const uint32_t b = moff[s], e = moff[s + 1];
            for (uint32_t i = b + (WAVE ? lane : 0u); i < e; i += WAVE ? 64u : 1u) atomicAdd(counts + mpid[i], v);
            if (!WAVE || lane == 0) mine = v * (e - b);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if (lane == 0 && mine) atomicAdd(total, mine);
}

// ---- records form: one thread per record; a run of one pattern over adjacent lanes becomes one add by its first lane
__global__ __launch_bounds__(kHxBlock) void k_hist_records(const acgpu_match* __restrict__ rec, uint64_t n, unsigned long long* __restrict__ counts,
                                                           uint64_t n_counts) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t i = uint64_t(blockIdx.x) * kHxBlock + threadIdx.x;
    const uint32_t pid = i < n ? rec[i].pattern : 0xFFFFFFFFu;   // (pattern ids stay below 2^31)
    const uint32_t prev = uint32_t(__shfl_up(int(pid), 1, 64));
    const bool head = lane == 0 || prev != pid;
    const uint64_t heads = __ballot(head);
    if (head && pid < n_counts) {
        const uint64_t later = lane == 63 ? 0 : heads >> (lane + 1);
        const uint32_t run = later ? uint32_t(__ffsll(static_cast<long long>(later))) : 64u - lane;
        atomicAdd(counts + pid, static_cast<unsigned long long>(run));
    }
}

__global__ void k_hist_zero(unsigned long long* a, uint64_t na, unsigned long long* b, uint64_t nb) {
    for (uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < na + nb; i += uint64_t(gridDim.x) * blockDim.x) {
        if (i < na) a[i] = 0; else b[i - na] = 0;
    }
}

template <int UP, int FLAV>
void lh_launch_cls(bool cc, dim3 grid, hipStream_t s, const LwArgs& la, const ScanGeom& g, const LwHistArgs& x) {
    const dim3 block{kLhBlock};
    if (cc) k_lw_hist<UP, FLAV, true><<<grid, block, 0, s>>>(la, g, x);
    else k_lw_hist<UP, FLAV, false><<<grid, block, 0, s>>>(la, g, x);
}
template <int UP>
void lh_launch(uint32_t flavour, bool cc, dim3 grid, hipStream_t s, const LwArgs& la, const ScanGeom& g, const LwHistArgs& x) {
    if (flavour == kLwFull) lh_launch_cls<UP, kLwFull>(cc, grid, s, la, g, x);
    else if (flavour == kLwWide) lh_launch_cls<UP, kLwWide>(cc, grid, s, la, g, x);
    else lh_launch_cls<UP, kLwNarrow>(cc, grid, s, la, g, x);
}

}  // namespace

hipError_t launch_lw_hist(const HotTables& h, const ScanGeom& g, unsigned long long* visits, hipStream_t s, bool agree) {
    if (!h.lw_ready || !visits) return hipErrorInvalidValue;
    const LwHostTables& t = h.lw;
    LwArgs la = lw_args(h);
    const int up = lw_lane_geometry(h, g, la);   // the lane-chunk rules of launch_hot_count
    if (la.n_tasks == 0 || h.hist_states == 0) return hipSuccess;
    if (h.lw_image_bytes > kLwLdsBytes) return hipErrorInvalidValue;
    const uint64_t blocks = lw_walk_blocks(la);
    LwHistArgs x{};
    x.visits = visits;
    x.n_bins = h.hist_states;
    x.agree = agree ? 1u : 0u;
    x.first_match = t.first_match;
    x.full_recip = t.flavour == kLwFull ? uint32_t((uint64_t(1) << 32) / t.row_bytes + 1) : 0u;
    // LDS bins: they fit behind the image, and no workgroup can be handed 2^32 bytes (see the head of the file)
    const uint32_t bins_off = (h.lw_image_bytes + 15u) & ~15u;
    const uint64_t tasks_per_wave = (la.n_tasks + blocks * kLhWaves - 1) / (blocks * kLhWaves);
    const uint64_t wg_bytes = tasks_per_wave * kLhWaves * 64 * uint64_t(la.lane_chunk);
    if (uint64_t(bins_off) + 4ull * x.n_bins <= kLwLdsBytes && wg_bytes < (uint64_t(1) << 32) - 1) x.bins_off = bins_off;
    const dim3 grid{uint32_t(blocks)};
    if (up == 4) lh_launch<4>(t.flavour, t.computed_cls, grid, s, la, g, x);
    else lh_launch<8>(t.flavour, t.computed_cls, grid, s, la, g, x);
    return hipGetLastError();
}

hipError_t launch_hist_expand(const HotTables& h, const unsigned long long* visits, unsigned long long* counts, unsigned long long* total, hipStream_t s) {
    if (!h.lw_ready || !h.hist_moff) return hipErrorInvalidValue;
    if (h.hist_states == 0) return hipSuccess;
    const bool wave = h.hist_max_list >= 32;   // long lists: the 64 lanes of a wavefront share one state's list
    const uint64_t threads = uint64_t(h.hist_states) * (wave ? 64 : 1);
    const dim3 grid{uint32_t((threads + kHxBlock - 1) / kHxBlock)}, block{kHxBlock};
    if (wave) k_hist_expand<true><<<grid, block, 0, s>>>(visits, h.hist_moff, h.hist_mpid, h.hist_states, counts, total);
    else k_hist_expand<false><<<grid, block, 0, s>>>(visits, h.hist_moff, h.hist_mpid, h.hist_states, counts, total);
    return hipGetLastError();
}

hipError_t launch_hist_records(const acgpu_match* records, uint64_t n, unsigned long long* counts, uint64_t n_counts, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + kHxBlock - 1) / kHxBlock;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    k_hist_records<<<dim3(uint32_t(blocks)), dim3(kHxBlock), 0, s>>>(records, n, counts, n_counts);
    return hipGetLastError();
}

hipError_t launch_hist_zero(unsigned long long* a, uint64_t na, unsigned long long* b, uint64_t nb, hipStream_t s) {
    if (na + nb == 0) return hipSuccess;
    const uint32_t blocks = uint32_t(std::min<uint64_t>((na + nb + 255) / 256, 1024));
    k_hist_zero<<<dim3(blocks), dim3(256), 0, s>>>(a, na, b, nb);
    return hipGetLastError();
}

}  // namespace acgpu

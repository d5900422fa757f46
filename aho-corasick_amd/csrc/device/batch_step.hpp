// Steppers of the batched searches (batch_find.hip, batch_iter.hip): start / next / is_special / is_match as the engines of
// engines.hpp, + the patterns of a match state.  One skeleton per kernel, the stepper a template parameter: the LDS rows of
// host/batch_tables.hpp -- one class lookup and one ds_read_u16 per byte --, DfaEng and CnfaEng on the global tables.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "batch_find.hpp"
#include "engines.hpp"

namespace acgpu {
namespace batchdev {

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t t = __shfl_xor(v, o, 64);
        v = t < v ? t : v;
    }
    return v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t t = __shfl_xor(v, o, 64);
        v = t > v ? t : v;
    }
    return v;
}

// The two places where a lane of try_find's loop (dev_try_find_fwd, kernels.hip; src/automaton.rs:1285-1420) looks at more
// than the next state, as k_batch_find has them in its tile walk -- for the other walks of a segment (the resolve of
// batch_long.hip).  k_batch_find itself keeps the text in place: called from here, the same statements inline to another
// register allocation (56 / 56 / 53 VGPR instead of 58 / 59 / 53), and that kernel's measured code is not to change for a
// helper's sake.  Positions are virtual; vb is the segment's begin (what an anchored match must start at).  Both return true
// when the lane is finished (a match under earliest semantics).
//
// before the first byte: a match at the start state (an empty pattern)
template <class S>
__device__ __forceinline__ bool lane_begin(const S& st, bool earliest, uint64_t at, uint32_t sid, bool& found, uint32_t& m_pid,
                                           uint64_t& m_start, uint64_t& m_end) {
    if (!st.is_match(sid)) return false;
    uint32_t pid, plen;
    st.first(sid, pid, plen);
    m_pid = pid; m_end = at; m_start = at - plen;
    found = true;
    return earliest;
}
// behind a byte that led to the match state `sid`; me: the position behind that byte
template <class S>
__device__ __forceinline__ bool lane_match(const S& st, bool anchored, bool earliest, uint64_t vb, uint64_t me, uint32_t sid,
                                           bool& found, uint32_t& m_pid, uint64_t& m_start, uint64_t& m_end) {
    uint32_t pid, plen;
    st.first(sid, pid, plen);
    const uint64_t ms = me - plen;
    if (anchored && ms > vb) return false;
    m_pid = pid; m_start = ms; m_end = me;
    found = true;
    return earliest;
}

template <class E>
struct GlobalStep {
    E eng;
    __device__ __forceinline__ void bind(const uint8_t* lds, const uint8_t* cls) { eng.cls = cls; }
    __device__ __forceinline__ uint32_t image_bytes() const { return 0; }
    __device__ __forceinline__ const void* image() const { return nullptr; }
    __device__ __forceinline__ const uint8_t* classes() const { return eng.cls; }
    __device__ __forceinline__ uint32_t start(bool anchored) const { return eng.start(anchored); }
    __device__ __forceinline__ uint32_t next(bool anchored, uint32_t sid, uint8_t byte) const { return eng.next(anchored, sid, byte); }
    __device__ __forceinline__ bool is_special(uint32_t sid) const { return eng.is_special(sid); }
    __device__ __forceinline__ bool is_match(uint32_t sid) const { return eng.is_match(sid); }
    __device__ __forceinline__ void first(uint32_t sid, uint32_t& pid, uint32_t& plen) const {
        pid = eng.match_pattern(sid, 0);
        plen = eng.pattern_len(pid);
    }
    // the whole match list of a match state, in list order (the overlapping iterator)
    __device__ __forceinline__ uint32_t list_len(uint32_t sid) const { return eng.match_len(sid); }
    __device__ __forceinline__ void list_at(uint32_t sid, uint32_t i, uint32_t& pid, uint32_t& plen) const {
        pid = eng.match_pattern(sid, i);
        plen = eng.pattern_len(pid);
    }
};

struct RowsStep {
    BatchRows t;
    const uint16_t* rows;   // LDS
    const uint8_t* cls;     // LDS
    __device__ __forceinline__ void bind(const uint8_t* lds, const uint8_t* c) { rows = reinterpret_cast<const uint16_t*>(lds); cls = c; }
    __device__ __forceinline__ uint32_t image_bytes() const { return t.rows_bytes; }
    __device__ __forceinline__ const void* image() const { return t.rows; }
    __device__ __forceinline__ const uint8_t* classes() const { return t.classes; }
    __device__ __forceinline__ uint32_t start(bool anchored) const { return anchored ? t.start_anchored : t.start_unanchored; }
    __device__ __forceinline__ uint32_t next(bool, uint32_t off, uint8_t byte) const { return rows[off + cls[byte]]; }
    __device__ __forceinline__ bool is_special(uint32_t off) const { return off <= t.max_special; }
    __device__ __forceinline__ bool is_match(uint32_t off) const { return off != kDevDead && off <= t.max_match; }
    __device__ __forceinline__ void first(uint32_t off, uint32_t& pid, uint32_t& plen) const {
        const uint2 v = *reinterpret_cast<const uint2*>(t.first + 2 * (off / t.alphabet_len - 2));
        pid = v.x;
        plen = v.y;
    }
};

// the rows with the match lists beside `first` (host/batch_tables.hpp): {offset, length} per match state into a flat
// array of {pattern id, pattern length}, global memory, read on the match path only
struct RowsListStep : RowsStep {
    const uint32_t* list_off;
    const uint32_t* list;
    __device__ __forceinline__ uint32_t list_len(uint32_t off) const { return list_off[2 * (off / t.alphabet_len - 2) + 1]; }
    __device__ __forceinline__ void list_at(uint32_t off, uint32_t i, uint32_t& pid, uint32_t& plen) const {
        const uint2 v = *reinterpret_cast<const uint2*>(list + 2 * (list_off[2 * (off / t.alphabet_len - 2)] + i));
        pid = v.x;
        plen = v.y;
    }
};

}  // namespace batchdev
}  // namespace acgpu

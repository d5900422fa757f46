// How the overlapping search sizes its event lists, its order pass and its chunk grids -- as PURE functions of a few
// integers, so that its two orchestrations (capi_overlap.cpp, capi_enqueue.cpp) cannot size one buffer by two rules and the
// rules can be tabulated on the host (tests/test_ov_sizes.py through acgpu_test_ov_sizes).  No HIP, no scratch.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace acgpu {

constexpr uint32_t kEvAllPairs = 16384;                  // events the all-pairs rank orders (k_ev_rank)
constexpr uint64_t kSortMaxEvents = uint64_t(12) << 20;  // events the bucket order pass takes (event_order.hip)

// Events the list of a prefix-filter scan over `span_bytes` holds: one per 64 haystack bytes, within [2^16, kSortMaxEvents].
inline uint64_t ov_event_capacity(uint64_t span_bytes) {
    return std::min<uint64_t>(kSortMaxEvents, std::max<uint64_t>(uint64_t(1) << 16, span_bytes / 64));
}

// What a scan and the order pass queued blind behind it are sized for.  `scan_cap` is the capacity the SCAN is launched
// with (the event list's); `events` / `records` bound the order pass: its scratch, its bucket size and the scan's
// histogram.  (A synchronous call that has read the counts back sizes the pass by the counts themselves.)
struct OvOrderBounds {
    uint64_t scan_cap = 0, events = 0, records = 0;
};
// ... for a guessed result size (find_iter's occurrence stream, capi_find.cpp): beyond the all-pairs rank's range, within
// the event list; the caller has room for `cap` records
inline OvOrderBounds ov_order_guessed(uint64_t span_bytes, uint64_t guess_events, uint64_t cap) {
    const uint64_t cap_ev = ov_event_capacity(span_bytes);
    return {cap_ev, std::min<uint64_t>(cap_ev, std::max<uint64_t>(guess_events, uint64_t(kEvAllPairs) + 1)), cap};
}
// ... with nothing but the density hint: whatever the event list holds, and the records that many events can plausibly
// stand for -- a handful of patterns per event -- never more than the caller has room for
inline OvOrderBounds ov_order_hinted(uint64_t span_bytes, uint64_t cap) {
    const uint64_t cap_ev = ov_event_capacity(span_bytes);
    return {cap_ev, cap_ev, std::min<uint64_t>({cap, uint64_t(1) << 26, 4 * cap_ev})};
}

// Bytes in front of a shard that a match ending in it may begin in; ScanGeom keeps it in 32 bits with room to spare.
inline size_t ov_halo(size_t max_pattern_len) { return max_pattern_len > 0 ? max_pattern_len - 1 : 0; }
inline bool ov_halo_ok(size_t halo) { return halo <= 0xFFFFFF00ull; }

// Chunk grid over the ownership window [emit_lo, emit_hi): origin at a multiple of `chunk`, at least one chunk.
inline uint64_t ov_grid_origin(uint64_t emit_lo, uint32_t chunk) { return (emit_lo / chunk) * chunk; }
inline uint64_t ov_grid_chunks(uint64_t emit_lo, uint64_t emit_hi, uint32_t chunk) {
    return std::max<uint64_t>(1, (emit_hi - ov_grid_origin(emit_lo, chunk) + chunk - 1) / chunk);
}
// the chunk fill behind an overflowed event form of the LDS walk: chunks of four lane-chunks (2 KiB: a wavefront per 512 bytes
// spends its time on warm-ups and prefix sums -- 1.5 ms against 1.2 for 92 M records)
constexpr uint32_t kLwFillStride = 4;
inline uint64_t ov_lw_fill_chunks(uint64_t n_lane_chunks) { return (n_lane_chunks + kLwFillStride - 1) / kLwFillStride; }

// May the LDS walk take its records from the events of its count walk (device/lds_emit.hip)?  Its event slabs take twice
// the searched span (lw_events_sizes): spans below 15 GiB.
inline bool ov_lw_events_eligible(bool lds_walk_first, bool variant_lw_events, size_t min_pattern_len, uint64_t span_bytes) {
    return lds_walk_first && variant_lw_events && min_pattern_len >= 1 && span_bytes < (uint64_t(15) << 30);
}

}  // namespace acgpu

// Launch wrappers of the device path for the long segments of the batched OVERLAPPING iterator (batch_iter_long.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "batch_iter.hpp"
#include "batch_long.hpp"

namespace acgpu {

// What the three kernels take beside the BatchIterArgs of the call and the BatchLongArgs of its long segments (wpre by
// launch_batch_long_scan, window, max_len).  A window has an id: wpre[entry] + its number within the segment.
struct BatchIterLongArgs {
    uint32_t* lane_cnt;     // [cap_windows * 64] records of lane l of window id: written by the count pass
    uint64_t* wsum;         // [cap_windows] count pass: the window's records; prefix pass: those of the segment's windows before it
    uint64_t cap_windows;   // what the two arrays hold: no kernel serves a window id at or beyond it
};

// count pass: lane_cnt, wsum.  form / rows: what plan_batch_iter chose; blocks: 0 = as many as the device holds
hipError_t launch_batch_iter_long_count(uint32_t form, const DevAutomaton& da, const BatchIterRows& rows, const BatchIterArgs& a,
                                        const BatchLongArgs& la, const BatchIterLongArgs& ila, uint32_t blocks, hipStream_t s);
// wsum: totals -> bases relative to the segment; counts[seg] = the segment's records; control word [2] = 1 when a segment
// has 2^32 records or more.  max_long: an upper bound of the entries (sizes the grid only)
hipError_t launch_batch_iter_long_prefix(const BatchIterArgs& a, const BatchLongArgs& la, const BatchIterLongArgs& ila, uint64_t max_long,
                                         hipStream_t s);
// fill pass: the records of window id to out[rec_off[seg] + wsum[id] ...), a lane's part at the prefix of lane_cnt
hipError_t launch_batch_iter_long_fill(uint32_t form, const DevAutomaton& da, const BatchIterRows& rows, const BatchIterArgs& a,
                                       const BatchLongArgs& la, const BatchIterLongArgs& ila, uint32_t blocks, hipStream_t s);

}  // namespace acgpu

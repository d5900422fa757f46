// Launch wrappers of the batched iterator (batch_iter.hip): every match of every segment of a packed haystack, CSR output.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "batch_find.hpp"

namespace acgpu {

// What the two passes take beside the BatchArgs of the batched find (whose `out` is the flat record array here; control
// word [2] is not used).
struct BatchIterArgs {
    BatchArgs b;
    uint32_t* counts;          // [n_seg] records per segment: written by the count pass (0 for a long segment)
    const uint64_t* rec_off;   // [n_seg + 1] their exclusive prefix: read by the fill pass
    int32_t overlapping;
};

// the LDS image with the match lists of its match states (host/batch_tables.hpp)
struct BatchIterRows {
    BatchRows r;
    const uint32_t* list_off;   // {offset, length} per match state
    const uint32_t* list;       // {pattern id, pattern length}, flat
};

// form: 1 DfaEng | 2 CnfaEng | 3 the LDS rows (BatchForm, as plan_batch_iter chose it); blocks: 0 = as many as the device holds
hipError_t launch_batch_iter_count(uint32_t form, const DevAutomaton& da, const BatchIterRows& rows, const BatchIterArgs& a,
                                   uint32_t blocks, hipStream_t s);
hipError_t launch_batch_iter_fill(uint32_t form, const DevAutomaton& da, const BatchIterRows& rows, const BatchIterArgs& a,
                                  uint32_t blocks, hipStream_t s);
// rec_off[n_seg] = the scan's total (launch_scan writes the n_seg exclusive offsets and totals[0])
hipError_t launch_batch_iter_seal(const uint64_t* totals, uint64_t* rec_off_end, hipStream_t s);

}  // namespace acgpu

// Launch wrappers of the device path for the long segments of the batched find (batch_long.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "batch_find.hpp"

namespace acgpu {

// What the three kernels take beside the BatchArgs of the call (whose ctl[1], longs and lkey the classify kernel has filled
// by the time they run).
struct BatchLongArgs {
    uint64_t* wpre;        // [longs_cap + 1] exclusive prefix of the entries' window counts, wpre[n_long] = their total
    uint32_t window;       // bytes of a segment whose match ends one wavefront task owns (batch_long_window)
    uint32_t max_len;      // max_pattern_len
    int32_t leftmost;      // the key is the smallest START of an occurrence (0: the smallest END -- the Standard rule)
    int32_t scouted;       // resolve: the keys were taken (0: every segment is walked from its begin)
};

// windows per entry -> wpre (one workgroup; the number of entries is read on the device)
hipError_t launch_batch_long_scan(const BatchArgs& a, const BatchLongArgs& la, hipStream_t s);
// the scout over the Standard automaton `da` of the patterns; form / rows: what plan_batch chose for THAT automaton.
// max_windows: an upper bound of the total the host can give (sizes the grid only); blocks: 0 = what the device holds
hipError_t launch_batch_scout(uint32_t form, const DevAutomaton& da, const BatchRows& rows, const BatchArgs& a, const BatchLongArgs& la,
                              uint64_t max_windows, uint32_t blocks, hipStream_t s);
// the lane loop from every entry's p* on the global tables of the automaton itself; max_long: upper bound of the entries
hipError_t launch_batch_resolve(const DevAutomaton& da, const BatchArgs& a, const BatchLongArgs& la, uint64_t max_long, hipStream_t s);

}  // namespace acgpu

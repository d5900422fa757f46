// Launch wrappers of the batched find (batch_find.hip): first match of every segment of a packed haystack.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "acgpu.h"
#include "kernels.hpp"

namespace acgpu {

// Control words of one call (device): the classify kernel and the walk report through them.
//   [0] lowest index of a segment whose offsets decrease or pass the haystack (UINT64_MAX: none)
//   [1] number of segments longer than lane_max (they are listed, not walked)
//   [2] number of walked segments with a match
constexpr int kBatchCtlWords = 3;
struct BatchLong { uint64_t seg, begin, end; };   // an entry of the list of long segments

struct BatchArgs {
    const uint8_t* hay16;      // haystack pointer rounded down to 16 B
    uint64_t mis;              // hay - hay16: positions below are virtual, v = haystack offset + mis
    uint64_t hay_len;
    const uint64_t* off;       // [n_seg + 1] (device)
    uint64_t n_seg;
    acgpu_match* out;          // [n_seg] (device)
    unsigned long long* ctl;   // [kBatchCtlWords]
    BatchLong* longs;          // [longs_cap]
    uint64_t longs_cap;
    unsigned long long* lkey;  // [longs_cap] or nullptr: a key per entry of that list, set to UINT64_MAX with the entry (batch_long.hpp)
    uint32_t lane_max;
    int32_t anchored, earliest;   // (earliest: already true for a Standard automaton)
#ifdef ACGPU_GUARD
    unsigned long long* guard;
    uint64_t guard_lo, guard_hi;
#endif
};

// the LDS image (host/batch_tables.hpp) as the kernel takes it
struct BatchRows {
    const uint16_t* rows;      // global; copied into LDS by every workgroup
    const uint32_t* first;     // {pattern id, length} per match state
    const uint8_t* classes;    // [256]
    uint32_t rows_bytes, alphabet_len;
    uint32_t start_unanchored, start_anchored, max_special, max_match;
};

// init of the control words + classification of the segments (validation, list of the long ones)
hipError_t launch_batch_classify(const BatchArgs& a, hipStream_t s);
// the walk; form: 1 DfaEng | 2 CnfaEng | 3 the LDS rows (BatchForm); blocks: 0 = as many as the device holds
hipError_t launch_batch_find(uint32_t form, const DevAutomaton& da, const BatchRows& rows, const BatchArgs& a, uint32_t blocks,
                             hipStream_t s);

}  // namespace acgpu

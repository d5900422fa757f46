// LDS image of the batched find's rows form (device/batch_find.hip, acgpu_find_batch): the automaton's OWN DFA -- its own
// start states, its own match kind, the reference's order of special states (dead, fail, match states, start states:
// src/dfa.rs:617-724) -- re-encoded as u16 rows.
//
//   rows[i * alphabet_len + c]   = (index of the next state of state i on class c) * alphabet_len: the premultiplied row
//                                  offset, so a step is rows[off + cls[byte]] and nothing else.  Offsets are monotone in the
//                                  state ids, so is_special / is_match stay compares against two of them.
//   first[(off / alphabet_len) - 2] = {first pattern id of that match state, its length}: what a match record needs, read on
//                                  the match path only (global memory).
//   list_off[2 * m], [2 * m + 1]  = {offset, length} of match state m's whole match list in `list`, a flat array of
//                                  {pattern id, pattern length} in list order: what the overlapping form of the batched
//                                  iterator (device/batch_iter.hip) reports at a match state; global memory as well.
//
// Built once per upload when batch_rows_fit (host/engine_plan.hpp) says the rows fit beside the staging tiles.
#pragma once
#include <cstdint>
#include <vector>

#include "automaton.hpp"
#include "devbuf.hpp"

namespace acgpu {

struct BatchImage {
    std::vector<uint16_t> rows;      // [states * alphabet_len], padded with zeros to a multiple of 8 entries (16 bytes)
    std::vector<uint32_t> first;     // [2 * match states]: pattern id, pattern length
    std::vector<uint32_t> list_off;  // [2 * match states]: offset into `list` (in pairs), length
    std::vector<uint32_t> list;      // [2 * sum of the lengths]: pattern id, pattern length
    uint32_t alphabet_len = 0;
    uint32_t start_unanchored = 0, start_anchored = 0, max_special = 0, max_match = 0;   // row offsets
};

// false: the DFA does not fit the image (nothing is written)
bool build_batch_image(const Dfa& d, const std::vector<uint32_t>& pattern_lens, BatchImage& out);

// the image on a device
struct BatchTables {
    bool ready = false;
    DevBuf rows, first, list_off, list;
    uint32_t rows_bytes = 0;     // multiple of 16
    uint32_t alphabet_len = 0;
    uint32_t start_unanchored = 0, start_anchored = 0, max_special = 0, max_match = 0;
    uint64_t dfa_states = 0;     // facts of plan_batch, whether or not the image was built
};
hipError_t upload_batch_tables(const Dfa& d, const std::vector<uint32_t>& pattern_lens, bool want_rows, BatchTables& out);

}  // namespace acgpu

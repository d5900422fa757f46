// Which engine a search starts with, which one it may be handed to, and what the adaptive hints of an automaton change
// about that -- as PURE functions of a handful of facts, so that the routing rules of capi_overlap.cpp (overlapping_impl and the
// enqueue-only form share them) can be tabulated and tested on the host (tests/test_engine_plan.py through
// acgpu_test_engine_plan).  Every engine returns identical results; the plan only decides cost.
#pragma once
#include <cstddef>
#include <cstdint>

namespace acgpu {

// (numbering of device/kernels.hpp: EngineId, + the prefix filter's other kernel, reported as the prefix filter)
constexpr uint32_t kPlanDfaWalk = 1, kPlanCnfaWalk = 2, kPlanLdsWalk = 3, kPlanPrefixFilter = 4, kPlanLargeSetFilter = 100;

struct EngineFacts {
    bool has_dfa = false;        // the device holds a full DFA of the automaton (its own, or derived at upload)
    bool pf_ready = false;       // prefix-filter tables (no empty pattern, <= 131 072 patterns, <= 2^20 states)
    bool lw_ready = false;       // the automaton fits the LDS walk
    bool lw_full = false;        // ... in its one-row-per-state form with the match lists in LDS: the reference's walk word for word,
                                 // the same speed whatever the match density, records from its events (device/lds_emit.hip)
    bool pfx_ready = false;      // large-set filter tables (>= 256 patterns, every pattern >= 4 bytes)
    size_t min_pattern_len = 0;
    int want = 0;                // acgpu_config.engine as the pipelines test it: 0 auto, 1 transition walk, 2 LDS walk, 3 prefix filter
    bool routing = true;         // variant `routing`
    bool count_hist = true;      // variant `count_hist` (pattern counts only)
};

struct EnginePlan {
    uint32_t first = 0;          // engine of the first scan; 0 = the requested engine is unavailable (ACGPU_ERR_INVALID_ARGUMENT)
    uint32_t alternative = 0;    // engine an abandoned prefix-filter scan is handed to (automatic choice only); 0 = none
};

inline EnginePlan plan_engines(const EngineFacts& f) {
    EnginePlan p;
    p.first = f.has_dfa ? kPlanDfaWalk : kPlanCnfaWalk;
    if (f.has_dfa) {
        // small automata: the transition walk from LDS first.  The prefix filter is 15 % faster on match-free input and up to
        // 20x slower where the patterns occur (profiles/r06_call_timelines_before.txt: 1.5 ms of a 256 MiB scan before its
        // routing rule gives up); the walk does not care
        if (f.want == 0 && f.lw_ready && f.lw_full && f.min_pattern_len > 0) p.first = kPlanLdsWalk;
        else if ((f.want == 0 || f.want == 3) && f.pf_ready) p.first = kPlanPrefixFilter;
        // (with an empty pattern every state is a match state: the LDS walk is not offered automatically)
        else if (((f.want == 0 && f.min_pattern_len > 0) || f.want == 2) && f.lw_ready) p.first = kPlanLdsWalk;
    }
    if ((f.want == 2 && p.first != kPlanLdsWalk) || (f.want == 3 && p.first != kPlanPrefixFilter)) { p.first = 0; return p; }
    if (p.first == kPlanPrefixFilter && f.want == 0 && f.routing) {
        if (f.lw_ready && f.min_pattern_len > 0) p.alternative = kPlanLdsWalk;
        else if (f.pfx_ready) p.alternative = kPlanLargeSetFilter;   // (automata too large for LDS)
        else if (f.has_dfa) p.alternative = kPlanDfaWalk;
    }
    return p;
}

// How acgpu_count_patterns gets its per-pattern counts (capi_count.cpp): from the visits of the match states, counted by the
// LDS walk and expanded through the match lists once per call (device/lds_hist.hip), or from the records of the
// overlapping search, whatever engine produces them.  The state-visit form needs the LDS image, no empty pattern (every
// state would be a match state: the LDS walk is not offered automatically there either), and an engine request it can
// honour; variant count_hist = 0 forces the records form.  A split set is asked with lw_ready = false (it has no image of
// its own).  Measured: profiles/count_hist_ab.txt.
enum class CountForm : uint32_t { Records = 0, StateVisits = 1 };
inline CountForm plan_count(const EngineFacts& f) {
    const bool engine_ok = f.want == 0 || f.want == 2;   // AUTO or LDS_WALK
    return f.lw_ready && f.min_pattern_len > 0 && engine_ok && f.count_hist ? CountForm::StateVisits : CountForm::Records;
}

// Which stepper the batched find walks with (acgpu_find_batch, capi_batch.cpp / device/batch_find.hip).  The workgroup has
// kBatchWaves wavefronts with a staging tile of kBatchTile bytes each and a 256-byte class map; what is left of the 160 KiB
// of LDS holds the automaton's own DFA as u16 rows of alphabet_len entries, every entry the PREMULTIPLIED row offset of the
// next state -- so the image is limited by its entry count (65 408 entries; the offsets then fit 16 bits as well).  Automata
// beyond that, and variant batch_rows = 0, walk the global tables: the DFA the device holds, else the contiguous NFA.
constexpr uint32_t kBatchTile = 8192, kBatchWaves = 4, kBatchLdsBytes = 160 * 1024;
constexpr uint32_t kBatchRowsMaxEntries = (kBatchLdsBytes - kBatchWaves * kBatchTile - 256) / 2;
constexpr uint32_t kBatchLaneMaxDefault = 4 * kBatchTile;   // variant batch_lane_max = 0
struct BatchFacts {
    bool has_dfa = false;        // the device holds a DFA of the automaton itself (its own, or derived at upload)
    uint64_t dfa_states = 0;     // ... with this many states (dead and fail included)
    uint32_t alphabet_len = 0;   // ... and this many byte classes
    bool batch_rows = true;      // variant `batch_rows`
};
enum class BatchForm : uint32_t { DfaWalk = 1, CnfaWalk = 2, LdsRows = 3 };   // (numbered as acgpu_engine)
inline bool batch_rows_fit(uint64_t dfa_states, uint32_t alphabet_len) {
    return dfa_states > 0 && alphabet_len > 0 && dfa_states * alphabet_len <= kBatchRowsMaxEntries;
}
inline BatchForm plan_batch(const BatchFacts& f) {
    if (f.has_dfa && f.batch_rows && batch_rows_fit(f.dfa_states, f.alphabet_len)) return BatchForm::LdsRows;
    return f.has_dfa ? BatchForm::DfaWalk : BatchForm::CnfaWalk;
}

// Who serves the segments of a batched find that are longer than a lane walks (capi_batch.cpp / device/batch_long.hip;
// DESIGN.md 3.2d "Long segments").  The device form needs one position p* per segment from which the lane loop on the
// automaton's own tables reports the segment's answer within max_pattern_len bytes: the segment's begin for an anchored
// search or a set with an empty pattern (Resolve), else a minimum over the occurrences of the Standard automaton of the same
// patterns, taken by a scout kernel that streams windows of the segment through the walk's LDS tile (ScoutResolve).  A
// window and its warm-up of max_pattern_len - 1 bytes share that tile: patterns whose warm-up would take more than
// kBatchLongWarmMax of it, and patterns longer than a lane walks, keep the single-span calls (HostCalls).
constexpr uint32_t kBatchLongWarmMax = kBatchTile / 8;
struct BatchLongFacts {
    bool anchored = false;            // acgpu_input.anchored
    bool standard = true;             // the automaton's match kind is Standard
    bool has_twin = false;            // ... or it has a Standard twin of the same patterns (acgpu_automaton::occ)
    bool occ_anchored_only = false;   // start kind of the automaton the scout would walk (the twin, else the automaton itself)
    bool split = false;               // the automaton or its twin is a split set (searched through its parts)
    size_t n_patterns = 0, min_pattern_len = 0, max_pattern_len = 0;
    uint32_t lane_max = kBatchLaneMaxDefault;
    bool batch_long = true;           // variant `batch_long`
};
enum class BatchLongForm : uint32_t { HostCalls = 0, Resolve = 1, ScoutResolve = 2 };
inline BatchLongForm plan_batch_long(const BatchLongFacts& f) {
    if (!f.batch_long || f.split || f.max_pattern_len > f.lane_max) return BatchLongForm::HostCalls;
    if (f.anchored || (f.n_patterns > 0 && f.min_pattern_len == 0)) return BatchLongForm::Resolve;
    if (f.n_patterns == 0 || (!f.standard && !f.has_twin) || f.occ_anchored_only) return BatchLongForm::HostCalls;
    if (f.max_pattern_len - 1 > kBatchLongWarmMax) return BatchLongForm::HostCalls;
    return BatchLongForm::ScoutResolve;
}
// bytes of a long segment whose match ENDS one wavefront of the scout owns per tile: the tile less the 16-byte aligned hull
// of the warm-up, a multiple of 64 so that every lane owns a whole number of bytes (>= 64 under kBatchLongWarmMax)
inline uint32_t batch_long_window(size_t max_pattern_len) {
    const uint32_t hull = (uint32_t(max_pattern_len) - 1 + 15 + 15) & ~15u;
    return (kBatchTile - hull) & ~63u;
}
static_assert(((kBatchTile - ((kBatchLongWarmMax + 30) & ~15u)) & ~63u) >= 64 * 64, "a lane owns at least 64 bytes");

// Who serves the long segments of a batched iterator (capi_batch_iter.cpp / device/batch_iter_long.hip; DESIGN.md 3.2e "Long
// segments").  The OVERLAPPING iteration has a device form: its records depend on the end position and the state there
// alone, and the state is known max_pattern_len - 1 bytes into a walk from the start state, so the windows of the scout
// above each emit their own records (WindowWalk) -- under the scout's limits on the warm-up.  The non-overlapping iteration
// of every match kind restarts where the last match ended, a chain across windows: it keeps the single-span calls, as do
// split sets, sets without a pattern and variant batch_long = 0.
enum class BatchIterLongForm : uint32_t { HostCalls = 0, WindowWalk = 1 };
inline BatchIterLongForm plan_batch_iter_long(const BatchLongFacts& f, bool overlapping) {
    if (!overlapping || !f.batch_long || f.split || f.n_patterns == 0) return BatchIterLongForm::HostCalls;
    if (f.max_pattern_len > f.lane_max || f.max_pattern_len > kBatchLongWarmMax + 1) return BatchIterLongForm::HostCalls;
    return BatchIterLongForm::WindowWalk;
}

// Which stepper the batched iterator walks with (acgpu_find_iter_batch, capi_batch_iter.cpp / device/batch_iter.hip): plan_batch's
// answer, except that its fill pass keeps kBatchIterStage records per wavefront in LDS beside the tiles (a task's records
// are put together there and stored as one piece), so the rows form is chosen only when the image fits what that leaves of
// the 160 KiB; an automaton between the two limits walks the global DFA.
constexpr uint32_t kBatchIterStage = 128;                                        // records (24 bytes each) per wavefront
constexpr uint32_t kBatchIterStageBytes = kBatchWaves * kBatchIterStage * 24;    // 12 KiB per workgroup
constexpr uint32_t kBatchIterRowsMaxEntries = kBatchRowsMaxEntries - kBatchIterStageBytes / 2;
inline BatchForm plan_batch_iter(const BatchFacts& f) {
    const BatchForm p = plan_batch(f);
    if (p == BatchForm::LdsRows && f.dfa_states * f.alphabet_len > kBatchIterRowsMaxEntries) return BatchForm::DfaWalk;
    return p;
}

// What the hints of the automaton make of a prefix-filter scan that has an alternative (spans of kProbeMinSpan and more,
// and only while the first kernel is the two-type filter): take the alternative unasked, ask the probe first, or just scan.
enum class PfStart : uint32_t { Scan = 0, Probe = 1, TakeAlternative = 2 };
constexpr uint64_t kPlanProbeMinSpan = uint64_t(16) << 20;
inline PfStart plan_pf_start(const EnginePlan& p, int probe_skip, int route_hint, uint64_t span_bytes, bool first_kernel_is_large_set) {
    if (p.first != kPlanPrefixFilter || !p.alternative || span_bytes < kPlanProbeMinSpan || first_kernel_is_large_set) return PfStart::Scan;
    if (probe_skip > 0) return PfStart::TakeAlternative;   // the last four probes in a row chose it: the next 32 searches do not ask
    if (route_hint > 0) return PfStart::Probe;             // recent scans were abandoned
    return PfStart::Scan;
}

}  // namespace acgpu

// C ABI of libacgpu.so, per-pattern occurrence counts (acgpu_count_patterns): counts[p] = the number of records with pattern p
// the overlapping search returns for the same input and shard -- without writing, ordering or copying any record where the
// LDS walk serves the automaton (device/lds_hist.hip: state visits, expanded through the match lists once per call), and from
// the record stream of the overlapping search (internal mode, records left in scratch) everywhere else.  See capi.cpp.
#include "capi_impl.hpp"

using namespace acgpu;
using namespace acgpu_capi;

namespace {

// the facts plan_count is asked with (a split set has no LDS image of its own: both parts are searched and merged)
acgpu_status count_facts(acgpu_automaton* aut, DeviceState** ds, EngineFacts* f) {
    if (acgpu_status st = get_device_state(aut->part[0] ? aut->part[0].get() : aut, ds)) return st;
    *f = engine_facts(aut, *ds);
    if (aut->part[0]) f->lw_ready = false;
    return ACGPU_OK;
}

struct CountCtx {
    acgpu_automaton* aut;
    DeviceState* ds;
    Scratch* sc;
    const acgpu_input* in;
    size_t shard_begin, shard_end;
    unsigned long long* dcounts;   // device
    size_t n_counts;
    acgpu_profile* prof;
    hipStream_t stream;
};

// State-visit form: walk -> expansion; *total from the device word behind the visits.
acgpu_status count_by_visits(const CountCtx& c, uint64_t* total) {
    Scratch* sc = c.sc;
    const HotTables& hot = c.ds->hot;
    const size_t halo = ov_halo(c.aut->nnfa.max_pattern_len);
    if (!ov_halo_ok(halo)) return ACGPU_ERR_INVALID_ARGUMENT;
    const size_t need_lo = std::max(c.in->span_start, c.shard_begin >= halo ? c.shard_begin - halo : size_t(0));
    const uint8_t* dhay = nullptr;
    if (acgpu_status st = device_haystack(c.in, need_lo, c.shard_end, sc, c.stream, &dhay)) return st;
    const ScanGeom g = make_geom(c.aut, c.in, c.shard_begin, c.shard_end, dhay, halo);
    unsigned long long* visits = sc->hist.as<unsigned long long>();
    unsigned long long* dtotal = visits + hot.hist_states;
    if (c.prof) HIP_TRY(hipEventRecord(sc->ev[0], c.stream));
    HIP_TRY(launch_lw_hist(hot, g, visits, c.stream, c.ds->var.count_hist != 2));
    if (c.prof) HIP_TRY(hipEventRecord(sc->ev[1], c.stream));
    HIP_TRY(launch_hist_expand(hot, visits, c.dcounts, dtotal, c.stream));
    if (c.prof) HIP_TRY(hipEventRecord(sc->ev[2], c.stream));
    HIP_TRY(hipMemcpyAsync(sc->pinned, dtotal, sizeof(uint64_t), hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    *total = sc->pinned[0];
    if (c.prof) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, sc->ev[0], sc->ev[1])); c.prof->ms_scan = ms;
        HIP_TRY(hipEventElapsedTime(&ms, sc->ev[1], sc->ev[2])); c.prof->ms_fill = ms;
        HIP_TRY(hipEventElapsedTime(&ms, sc->ev[0], sc->ev[2])); c.prof->ms_total = ms;
        c.prof->bytes_scanned = c.shard_end - c.shard_begin;
        c.prof->n_chunks = g.n_chunks;
        c.prof->engine_used = ENG_HOT;
    }
    return ACGPU_OK;
}

// Records form: the overlapping search in its internal mode (ordered records left in this scratch), piece by piece so that the
// record stream of a dense input stays bounded, and one histogram launch per piece.  Consecutive shards tile the stream.
constexpr size_t kCountPiece = size_t(256) << 20;
acgpu_status count_by_records(const CountCtx& c, uint64_t* total) {
    Scratch* sc = c.sc;
    acgpu_input oin = *c.in;
    oin.out_on_device = 0;
    DenseRule rule;
    rule.guard = false;   // (there is no alternative to hand a dense stream to)
    *total = 0;
    for (size_t pb = c.shard_begin;;) {
        const size_t pe = std::min(c.shard_end, pb + kCountPiece);
        size_t n = 0;
        acgpu_match* rec = nullptr;
        acgpu_profile pp;
        if (acgpu_status st = overlapping_impl(c.aut, &oin, pb, pe, nullptr, 0, &n, c.prof ? &pp : nullptr, sc, &rec, &rule)) return st;
        if (n && !rec) return ACGPU_ERR_INVALID_ARGUMENT;
        if (c.prof) HIP_TRY(hipEventRecord(sc->ev[6], c.stream));
        HIP_TRY(launch_hist_records(rec, n, c.dcounts, c.n_counts, c.stream));
        if (c.prof) {
            HIP_TRY(hipEventRecord(sc->ev[7], c.stream));
            HIP_TRY(hipStreamSynchronize(c.stream));
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, sc->ev[6], sc->ev[7]));
            c.prof->ms_scan += pp.ms_total; c.prof->ms_fill += ms; c.prof->ms_total += pp.ms_total + ms;
            c.prof->bytes_scanned += pp.bytes_scanned; c.prof->n_chunks += pp.n_chunks;
            c.prof->engine_used = pp.engine_used; c.prof->routed |= pp.routed;
        }
        *total += n;
        if (pe >= c.shard_end) break;
        pb = pe;
    }
    HIP_TRY(hipStreamSynchronize(c.stream));   // (the scratch goes back to its pool)
    return ACGPU_OK;
}

}  // namespace

acgpu_status acgpu_count_plan_of(acgpu_automaton* aut, uint32_t* form) {
    if (!aut || !form) return ACGPU_ERR_INVALID_ARGUMENT;
    DeviceState* ds = nullptr;
    EngineFacts f;
    if (acgpu_status st = count_facts(aut, &ds, &f)) return st;
    *form = uint32_t(plan_count(f));
    return ACGPU_OK;
}

extern "C" acgpu_status acgpu_count_patterns(acgpu_automaton* aut, const acgpu_input* in, size_t shard_begin, size_t shard_end,
                                             uint64_t* counts, size_t n_counts, uint32_t flags, uint64_t* total, acgpu_profile* prof) {
    // ---- checks: those of the overlapping search in its order, then the count's own; all before any device work
    if (!aut) return ACGPU_ERR_INVALID_ARGUMENT;
    if (total) *total = 0;
    if (prof) std::memset(prof, 0, sizeof *prof);
    acgpu_automaton* target = nullptr;
    acgpu_status st = check_overlapping(aut, in, &target);
    if (st) return st;
    if (n_counts != acgpu_patterns_len(aut) || (n_counts && !counts)) {
        g_last_error = "acgpu_count_patterns: n_counts must be acgpu_patterns_len(aut) (" + std::to_string(acgpu_patterns_len(aut)) + "), got " + std::to_string(n_counts);
        return ACGPU_ERR_INVALID_ARGUMENT;
    }
    const bool accumulate = (flags & ACGPU_COUNT_ACCUMULATE) != 0;
    if ((flags & ~ACGPU_COUNT_ACCUMULATE) != 0 || (accumulate && !in->out_on_device)) {
        g_last_error = "acgpu_count_patterns: ACGPU_COUNT_ACCUMULATE is the only flag, and it needs device-resident counts";
        return ACGPU_ERR_INVALID_ARGUMENT;
    }
    const bool done = in->span_start > in->span_end;   // Input::is_done: no occurrence
    if (!done && !(in->span_start <= shard_begin && shard_begin <= shard_end && shard_end <= in->span_end)) return ACGPU_ERR_INVALID_ARGUMENT;
    if (done && !in->out_on_device) { std::fill(counts, counts + n_counts, uint64_t(0)); return ACGPU_OK; }
    aut = target;

    // ---- context
    CountCtx c{};
    EngineFacts facts;
    if ((st = count_facts(aut, &c.ds, &facts))) return st;
    ScratchLease lease(c.ds);
    Scratch* sc = lease.s.get();
    c.aut = aut; c.sc = sc; c.in = in; c.shard_begin = shard_begin; c.shard_end = shard_end; c.n_counts = n_counts; c.prof = prof;
    c.stream = static_cast<hipStream_t>(in->stream);
    if (prof && (st = ensure_events(sc))) return st;
    HIP_TRY(sc->ensure_pinned());
    const bool visits = !done && plan_count(facts) == CountForm::StateVisits;
    const size_t n_hist = visits ? size_t(c.ds->hot.hist_states) + 1 : 0;   // visits[] + the total word
    if (n_hist) HIP_TRY(sc->hist.ensure(n_hist * sizeof(uint64_t)));
    if (!in->out_on_device) HIP_TRY(sc->hcounts.ensure(std::max<size_t>(n_counts, 1) * sizeof(uint64_t)));
    c.dcounts = in->out_on_device ? reinterpret_cast<unsigned long long*>(counts) : sc->hcounts.as<unsigned long long>();
    HIP_TRY(launch_hist_zero(sc->hist.as<unsigned long long>(), n_hist, c.dcounts, accumulate ? 0 : n_counts, c.stream));

    uint64_t n_total = 0;
    if (!done && (st = visits ? count_by_visits(c, &n_total) : count_by_records(c, &n_total))) return st;
    if (!in->out_on_device && n_counts) HIP_TRY(hipMemcpyAsync(counts, c.dcounts, n_counts * sizeof(uint64_t), hipMemcpyDeviceToHost, c.stream));
    HIP_TRY(hipStreamSynchronize(c.stream));
    if (total) *total = n_total;
    if (prof) prof->n_matches = n_total;
    return ACGPU_OK;
}

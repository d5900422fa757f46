// C ABI of libacgpu.so, the enqueue-only overlapping search (acgpu_find_overlapping_enqueue*): everything queued on the caller's stream, sizes read
// on the device, no host round trip.  See capi.cpp.
#include "capi_impl.hpp"

using namespace acgpu;
using namespace acgpu_capi;

namespace {

// Everything one call needs, resolved once by enqueue_impl and shared by its three pipelines.
struct EnqCtx {
    acgpu_automaton* aut = nullptr;
    DeviceState* ds = nullptr;
    DeviceState::AsyncCtx* ctx = nullptr;
    Scratch* sc = nullptr;
    hipStream_t stream = nullptr;
    ScanGeom g{};
    size_t shard_begin = 0;
    uint64_t span_bytes = 0;
    uint32_t eng = 0;
    acgpu_match* out = nullptr;
    size_t cap = 0;
    uint64_t* totals = nullptr;
    int32_t slot = -1;
    uint32_t flags = 0;
    bool* probed = nullptr;
    EnqueueGuess* guess = nullptr;
    EnqueueSync* sync = nullptr;
    // the slot's events around the scan (none for slot < 0)
    hipError_t slot_begin() const { return slot >= 0 ? hipEventRecord(ctx->ev[2 * slot], stream) : hipSuccess; }
    hipError_t slot_end() const { return slot >= 0 ? hipEventRecord(ctx->ev[2 * slot + 1], stream) : hipSuccess; }
};

constexpr uint32_t kEvCap = ACGPU_ENQUEUE_MAX_EVENTS;
static_assert(kEvCap == kEvAllPairs, "the enqueue form orders its events with the all-pairs rank");

// Fused order chain (event_order.hip) while the automaton's recent results were dense: the scan does the histogram, the
// order pass serves ANY number of events, its last kernel reports the totals and re-arms the counters -- no
// all-pairs kernels, no copy -- and the bucket words are re-zeroed BEHIND it (natural text, 1 GiB: 13 launches behind
// the scan -> 4, 118 us -> ~50).  With the device-side probe both gated scans carry the histogram: one of them runs.
acgpu_status enqueue_pf_fused(EnqCtx& e, unsigned long long* ctr, PfRoute route, bool probe) {
    // (bounds: a guessed result size -- find_iter's occurrence e.stream, capi_find.cpp -- or what the event list holds)
    const OvOrderBounds ob = e.guess ? ov_order_guessed(e.span_bytes, e.guess->max_events, e.cap) : ov_order_hinted(e.span_bytes, e.cap);
    HIP_TRY(e.sc->order.reserve(event_order_work_bytes(ob.events, ob.records, e.span_bytes)));
    const size_t zb = event_order_zero_bytes(ob.events, ob.records, e.span_bytes);
    HIP_TRY(e.sc->order.zero(zb, e.stream));
    route.hist = event_order_hist(ob.events, ob.records, e.shard_begin, e.span_bytes, e.sc->order.buf.p);
    if (acgpu_status st = launch_pf_scan_pair(e.sc, e.ds->hot, e.g, e.span_bytes, ctr, ob.scan_cap, route, probe, e.stream)) return st;
    HIP_TRY(e.slot_end());
    EoFused fz;
    fz.ctr = ctr; fz.totals = e.totals; fz.host_totals = e.sync ? e.sync->host_totals : nullptr; fz.seq = e.sync ? e.sync->seq : 0;
    HIP_TRY(launch_event_order_emit(e.ds->hot, e.ds->da, e.sc->events.p, nullptr, 0, ob.events, ob.records, e.shard_begin, e.span_bytes, e.sc->order.buf.p,
                                    e.out, e.stream, nullptr, true, &fz));
    e.sc->ev_armed = true;   // (the chain's last kernel zeroes the counters; the rank words were not touched)
    if (e.guess) {   // (the caller queues its own kernels first, then the re-zeroing)
        e.guess->served_events = ob.events; e.guess->rearm_bytes = zb;
        return ACGPU_OK;
    }
    if (e.sync && e.sync->host_totals) {
        if (!e.ctx->fin) HIP_TRY(hipEventCreateWithFlags(&e.ctx->fin, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(e.ctx->fin, e.stream));
        e.sync->done = e.ctx->fin;
    }
    HIP_TRY(e.sc->order.rezero_behind(zb, e.stream));
    return ACGPU_OK;
}

// Prefix filter, sparse results (up to ACGPU_ENQUEUE_MAX_EVENTS occurrences): filter scan -> all-pairs rank -> ordered
// records; beyond that the bucket order pass takes over where a guess or the density hint had it queued.
acgpu_status enqueue_pf_events(EnqCtx& e) {
    acgpu_status st;
    const uint64_t cap_ev = ov_event_capacity(e.span_bytes);
    unsigned long long* ctr = nullptr;
    uint32_t* rank = nullptr;
    if ((st = arm_pf_events(e.sc, cap_ev, e.stream, &ctr, &rank))) return st;
    // the routing rule of the synchronous form applies here too: an abandoned scan reports totals[1] = UINT64_MAX,
    // which the caller treats like an event overflow ("repeat with the synchronous call": that one switches engine
    // and remembers).  While the automaton is remembered as "recently abandoned" and its alternative is the large-set
    // filter -- natural text against a dictionary -- the probe decides on the device: both filters are enqueued, gated
    // on the probe's word, one of them returns at once.
    PfRoute route;
    const uint32_t alt = pf_alternative(e.aut, e.ds, &route);
    EnginePlan plan;
    plan.first = ENG_PF; plan.alternative = alt;
    // (plan_pf_start for the large-set alternative only -- TakeAlternative: that filter unasked, Probe: the device-side probe; any other alternative needs a host decision)
    const PfStart how = alt == ENG_PF_LARGE ? plan_pf_start(plan, e.ds->probe_skip.load(std::memory_order_relaxed), e.ds->route_hint.load(std::memory_order_relaxed),
                                                            e.span_bytes, pf_uses_large_set(e.ds->hot, route))
                                            : PfStart::Scan;
    // (after four synchronous probes in a row that chose the large-set filter the next searches take it unasked)
    if (how == PfStart::TakeAlternative) { e.ds->probe_skip.fetch_sub(1, std::memory_order_relaxed); route = PfRoute(); route.force_pfx = true; }
    const bool probe = how == PfStart::Probe;
    if (probe) {
        if (e.probed) *e.probed = true;
        if ((st = ensure_probe(e.sc, e.stream))) return st;
        uint32_t* flag = reinterpret_cast<uint32_t*>(e.sc->probe.as<uint8_t>() + 64);
        HIP_TRY(launch_pf_probe(e.ds->hot, e.g, route, flag, e.sc->probe.as<unsigned long long>(), e.stream));
        route.gate = flag; route.gate_val = 0;
        HIP_TRY(e.slot_begin());   // (the slot times the scan, not the probe in front of it)
    }
    const bool room = e.out && e.cap;
    if (e.ds->var.eo_fused && room && (e.guess || e.ds->dense_hint.load(std::memory_order_relaxed) > 0)) {
        if (!e.guess) e.ds->dense_hint.fetch_sub(1, std::memory_order_relaxed);
        return enqueue_pf_fused(e, ctr, route, probe);
    }
    e.sc->order.dirty();   // (the chains below use the order pass's scratch their own way)
    if ((st = launch_pf_scan_pair(e.sc, e.ds->hot, e.g, e.span_bytes, ctr, cap_ev, route, probe, e.stream))) return st;
    HIP_TRY(e.slot_end());
    // (a guessed result size: the order pass below is certain to be queued -- its scratch is sized first, so that
    // k_ev_write can zero its counters on the way)
    OvOrderBounds gb;
    void* zero_p = nullptr;
    size_t zero_bytes = 0;
    if (e.guess && room) {
        gb = ov_order_guessed(e.span_bytes, e.guess->max_events, e.cap);
        HIP_TRY(e.sc->order.reserve(event_order_work_bytes(gb.events, gb.records, e.span_bytes)));
        zero_bytes = event_order_zero_bytes(gb.events, gb.records, e.span_bytes);
        if (zero_bytes <= (size_t(1) << 20)) zero_p = e.sc->order.buf.p; else zero_bytes = 0;
    }
    HIP_TRY(launch_pf_event_rank(e.sc->events.p, ctr, kEvCap, rank, e.totals, e.guess && e.guess->over_all_pairs ? 0u : kEvCap / 2, e.stream));   // (grid hint only: grid-stride kernel)
    HIP_TRY(launch_pf_event_write(e.ds->hot, e.ds->da, e.sc->events.p, ctr, kEvCap, rank, e.totals, e.out ? e.cap : 0, e.out, e.stream, zero_p, zero_bytes));
    e.sc->ev_armed = true;
    if (gb.events) {
        HIP_TRY(launch_event_order_emit(e.ds->hot, e.ds->da, e.sc->events.p, e.totals, kEvCap, gb.events, gb.records, e.shard_begin, e.span_bytes,
                                        e.sc->order.buf.p, e.out, e.stream, nullptr, zero_p != nullptr));
        e.guess->served_events = gb.events;
        return ACGPU_OK;
    }
    // more occurrences than the all-pairs rank orders: while the automaton's recent (synchronous) results were dense,
    // the bucket order pass is queued too -- launches that return at once unless needed -- and resets totals[1] to 0
    // when it delivered; otherwise the caller sees totals[1] > ACGPU_ENQUEUE_MAX_EVENTS and repeats synchronously
    if (room && e.ds->dense_hint.load(std::memory_order_relaxed) > 0) {
        e.ds->dense_hint.fetch_sub(1, std::memory_order_relaxed);
        // (if the pass's scratch cannot be had it is simply not queued: the scan and the all-pairs path above are already
        // enqueued, the caller sees totals[1] > MAX and repeats synchronously)
        const OvOrderBounds hb = ov_order_hinted(e.span_bytes, e.cap);
        const hipError_t oe = e.sc->order.reserve(event_order_work_bytes(hb.events, hb.records, e.span_bytes));
        if (oe == hipSuccess)
            HIP_TRY(launch_event_order_emit(e.ds->hot, e.ds->da, e.sc->events.p, e.totals, kEvCap, hb.events, hb.records, e.shard_begin, e.span_bytes,
                                            e.sc->order.buf.p, e.out, e.stream, e.totals));
        else { (void)hip_fail(oe, "order pass work area"); (void)hipGetLastError(); }   // (the message stays for acgpu_last_error)
    }
    return ACGPU_OK;
}

// the LDS walk of a small automaton: records from the events of its count walk (lds_emit.hip), the chunk fill gated on
// their overflow word -- everything reads its sizes on the device
acgpu_status enqueue_lw_events(EnqCtx& e, uint32_t lane_chunk) {
    const ScanGeom eg = with_chunk(e.g, lane_chunk);
    ScanScratch es;
    if (acgpu_status st = scan_scratch(e.sc, eg.n_chunks, true, &es)) return st;
    uint32_t gen = 0;
    if (acgpu_status st = ensure_lw_events(e.sc, eg, e.stream, &gen)) return st;
    uint32_t* ovf = e.sc->lwovf.as<uint32_t>();
    uint32_t* task_n = e.sc->lwtn.as<uint32_t>();
    HIP_TRY(launch_lw_count_ev(e.ds->hot, eg, es.counts, e.sc->lwev.p, task_n, ovf, gen, e.stream));
    HIP_TRY(e.slot_end());
    HIP_TRY(launch_lw_task_scan(eg, task_n, es.totals, nullptr, nullptr, e.stream));
    if (e.cap > 0 && e.out) {
        // the chunk fill (behind the lane-chunk scan it takes its offsets from: four launches, gated on the overflow word) is
        // queued while the automaton's recent results overflowed their slabs; otherwise an overflow is REPORTED
        // (totals[1] = UINT64_MAX: the caller repeats with the synchronous call, which remembers)
        const bool with_fill = e.ds->lw_dense_hint.load() > 0 || !e.ds->adaptive || (e.flags & ACGPU_ENQUEUE_CLASSIC) != 0;   // (classic: dense results asked for)
        HIP_TRY(launch_lw_ev_emit(e.ds->hot, eg, e.sc->lwev.p, task_n, ovf, gen, es.counts, es.totals, e.cap, e.out, e.stream, e.totals, !with_fill));
        if (with_fill) HIP_TRY(launch_lw_chunk_fill(e.ds->hot, eg, es, e.cap, 16384, e.out, ovf, gen, e.stream));
        return ACGPU_OK;
    }
    HIP_TRY(hipMemcpyAsync(e.totals, es.totals, sizeof(uint64_t), hipMemcpyDeviceToDevice, e.stream));
    HIP_TRY(hipMemsetAsync(e.totals + 1, 0, sizeof(uint64_t), e.stream));
    return ACGPU_OK;
}

// every other engine, and dense results on request (ACGPU_ENQUEUE_CLASSIC): chunk counters -> scan -> fill, all
// reading their sizes on the device -- no occurrence limit, no host round trip
acgpu_status enqueue_classic(EnqCtx& e) {
    acgpu_status st;
    ScanScratch ss;
    if ((st = scan_scratch(e.sc, e.g.n_chunks, false, &ss))) return st;
    TriEvents tev;
    if ((st = cnfa_tri_events(e.ds, e.sc, e.eng, e.g, e.span_bytes, e.stream, &tev, &ss))) return st;
    if (e.eng == ENG_PF) {
        PfRoute pfr;
        if ((st = pf_route_prepare(e.sc, e.ds->hot, e.span_bytes, &pfr))) return st;
        HIP_TRY(launch_pf_any(e.ds->hot, e.g, ss.counts, e.stream, nullptr, nullptr, 0, pfr));
    } else if (e.eng == ENG_HOT) HIP_TRY(launch_hot_count(e.ds->hot, e.ds->da, e.g, ss.counts, e.stream));
    else HIP_TRY(launch_generic_count(e.eng, e.ds, e.g, ss.counts, e.stream, &tev));
    HIP_TRY(e.slot_end());
    HIP_TRY(launch_scan(ss, e.g.n_chunks, e.stream));
    if (e.cap > 0 && e.out) HIP_TRY(launch_fill(e.aut, e.ds, e.eng, e.g, ss, tev, true, e.out, e.cap, 16384, e.stream));
    HIP_TRY(hipMemcpyAsync(e.totals, ss.totals, sizeof(uint64_t), hipMemcpyDeviceToDevice, e.stream));   // records
    HIP_TRY(hipMemsetAsync(e.totals + 1, 0, sizeof(uint64_t), e.stream));                                  // no event list, no event limit
    return ACGPU_OK;
}

}  // namespace

// slot 64 is the library's own (the synchronous call that borrows a stream's enqueue context times itself there, leaving
// the caller's slots 0..63 alone); *probed = whether THIS call queued the device-side probe
acgpu_status acgpu_capi::enqueue_impl(acgpu_automaton* aut, const acgpu_input* in, size_t shard_begin, size_t shard_end, acgpu_match* out,
                                      size_t cap, uint64_t* totals, int32_t slot, uint32_t flags, bool* probed, EnqueueGuess* guess,
                                      EnqueueSync* sync) {
    // ---- checks
    if (probed) *probed = false;
    if (sync) sync->done = nullptr;
    if (!aut || !totals || slot > 64) return ACGPU_ERR_INVALID_ARGUMENT;
    acgpu_automaton* target = nullptr;
    acgpu_status st = check_overlapping(aut, in, &target);
    if (st) return st;
    if (!(in->span_start <= shard_begin && shard_begin <= shard_end && shard_end <= in->span_end))
        return ACGPU_ERR_INVALID_ARGUMENT;
    if (target != aut) return enqueue_impl(target, in, shard_begin, shard_end, out, cap, totals, slot, flags, probed, guess, sync);
    EnqCtx e;
    if ((st = get_device_state(aut, &e.ds))) return st;
    if (!in->haystack_on_device || !(cap == 0 || out)) {
        g_last_error = "enqueue form: device haystack and device output required";
        return ACGPU_ERR_INVALID_ARGUMENT;
    }
    const size_t halo = ov_halo(aut->nnfa.max_pattern_len);
    if (!ov_halo_ok(halo)) return ACGPU_ERR_INVALID_ARGUMENT;
    e.eng = plan_engines(engine_facts(aut, e.ds)).first;   // (host/engine_plan.hpp; no routing target is needed here: enqueue_pf_events)
    if (e.eng == 0) {
        g_last_error = "requested engine is unavailable for this automaton";
        return ACGPU_ERR_INVALID_ARGUMENT;
    }
    // ---- context
    e.aut = aut; e.stream = static_cast<hipStream_t>(in->stream);
    e.ctx = e.ds->async_ctx(e.stream);
    e.sc = &e.ctx->sc;
    e.g = make_geom(aut, in, shard_begin, shard_end, in->haystack, halo);
    e.shard_begin = shard_begin; e.span_bytes = e.g.emit_hi - e.g.emit_lo;
    e.out = out; e.cap = cap; e.totals = totals; e.slot = slot; e.flags = flags; e.probed = probed; e.guess = guess; e.sync = sync;
    if (slot >= 0) for (int k = 0; k < 2; k++) if (!e.ctx->ev[2 * slot + k]) HIP_TRY(hipEventCreate(&e.ctx->ev[2 * slot + k]));
    HIP_TRY(e.slot_begin());
    if (aut->part[0]) {
        // a split pattern set has no enqueue-only form (two pipelines and a merge sized from their counts): the call reports
        // "more occurrences than this form delivers", on which callers repeat with the synchronous call (acgpu.h) -- behind the
        // argument checks above, with the slot's events recorded like any other call
        HIP_TRY(hipMemsetAsync(totals, 0, sizeof(uint64_t), e.stream));
        HIP_TRY(hipMemsetAsync(totals + 1, 0xFF, sizeof(uint64_t), e.stream));
        HIP_TRY(e.slot_end());
        return ACGPU_OK;
    }
    if (in->span_start > in->span_end) {   // Input::is_done: no matches
        HIP_TRY(hipMemsetAsync(totals, 0, 2 * sizeof(uint64_t), e.stream));
        HIP_TRY(e.slot_end());
        return ACGPU_OK;
    }
    // ---- the pipeline
    if (e.eng == ENG_PF && aut->nnfa.max_pattern_len <= 0xFFFF && !(flags & ACGPU_ENQUEUE_CLASSIC)) return enqueue_pf_events(e);
    if (const uint32_t lane_chunk = lw_events_lane_chunk(aut, e.ds, e.eng, e.g)) return enqueue_lw_events(e, lane_chunk);
    return enqueue_classic(e);
}

extern "C" {
acgpu_status acgpu_find_overlapping_enqueue_ex(acgpu_automaton* aut, const acgpu_input* in, size_t shard_begin,
                                               size_t shard_end, acgpu_match* out, size_t cap, uint64_t* totals,
                                               int32_t slot, uint32_t flags) {
    if (slot >= 64) return ACGPU_ERR_INVALID_ARGUMENT;
    return enqueue_impl(aut, in, shard_begin, shard_end, out, cap, totals, slot, flags, nullptr);
}

acgpu_status acgpu_find_overlapping_enqueue(acgpu_automaton* aut, const acgpu_input* in, size_t shard_begin,
                                            size_t shard_end, acgpu_match* out, size_t cap, uint64_t* totals,
                                            int32_t slot) {
    return acgpu_find_overlapping_enqueue_ex(aut, in, shard_begin, shard_end, out, cap, totals, slot, 0);
}

acgpu_status acgpu_enqueue_kernel_ms(acgpu_automaton* aut, void* stream, int32_t slot, float* ms) {
    if (!aut || !ms || slot < 0 || slot >= 64) return ACGPU_ERR_INVALID_ARGUMENT;
    if (aut->cfg.start_kind == ACGPU_START_BOTH && aut->occ) return acgpu_enqueue_kernel_ms(aut->occ.get(), stream, slot, ms);
    DeviceState* ds = nullptr;
    acgpu_status st = get_device_state(aut, &ds);
    if (st) return st;
    DeviceState::AsyncCtx* ctx = ds->async_ctx(static_cast<hipStream_t>(stream));
    if (!ctx->ev[2 * slot] || !ctx->ev[2 * slot + 1]) return ACGPU_ERR_INVALID_ARGUMENT;
    HIP_TRY(hipEventElapsedTime(ms, ctx->ev[2 * slot], ctx->ev[2 * slot + 1]));
    return ACGPU_OK;
}

}  // extern "C"

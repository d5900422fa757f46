// C ABI of libacgpu.so, batched find (acgpu_find_batch): the first match of every segment of a packed haystack, one call
// for millions of short texts.  Three launches (control words, classify, walk: device/batch_find.hip), three more for the
// segments too long for a lane where the call may have any (window-count scan, scout, resolve: device/batch_long.hip), and ONE
// synchronisation, in which the host reads the offsets' error flag.  Where plan_batch_long keeps the long segments off the
// device, the host reads their list as well and serves them one by one by acgpu_find on their span.  See capi.cpp.
#include "capi_impl.hpp"

using namespace acgpu;
using namespace acgpu_capi;

namespace acgpu_capi {

#ifdef ACGPU_GUARD
unsigned long long* guard_counter();   // capi.cpp
#endif

// the inputs of plan_batch_long for this call
BatchLongFacts batch_long_facts(const acgpu_automaton* aut, const acgpu_input* in, uint32_t lane_max) {
    const acgpu_automaton* o = aut->occ ? aut->occ.get() : aut;
    BatchLongFacts f;
    f.anchored = in->anchored != 0;
    f.standard = aut->cfg.match_kind == ACGPU_MATCH_STANDARD;
    f.has_twin = bool(aut->occ);
    f.occ_anchored_only = o->cfg.start_kind == ACGPU_START_ANCHORED;
    f.split = aut->part[0] || o->part[0];
    f.n_patterns = aut->nnfa.pattern_lens.size();
    f.min_pattern_len = aut->nnfa.min_pattern_len;
    f.max_pattern_len = aut->nnfa.max_pattern_len;
    f.lane_max = lane_max;
    f.batch_long = aut->var.batch_long != 0;
    return f;
}

BatchRows batch_rows_of(const DeviceState* ds) {
    const BatchTables& t = ds->batch;
    BatchRows rows{};
    rows.rows = t.rows.as<uint16_t>(); rows.first = t.first.as<uint32_t>(); rows.classes = ds->da.dfa.classes;
    rows.rows_bytes = t.rows_bytes; rows.alphabet_len = t.alphabet_len;
    rows.start_unanchored = t.start_unanchored; rows.start_anchored = t.start_anchored;
    rows.max_special = t.max_special; rows.max_match = t.max_match;
    return rows;
}

BatchFacts batch_facts(const DeviceState* ds) {
    BatchFacts f;
    f.has_dfa = ds->da.has_dfa;
    f.dfa_states = ds->batch.dfa_states;
    f.alphabet_len = ds->batch.alphabet_len;
    f.batch_rows = ds->var.batch_rows != 0 && ds->batch.ready;
    return f;
}

std::string batch_bad_offsets_text(uint64_t seg) {
    return "offsets[" + std::to_string(seg + 1) + "] is below offsets[" + std::to_string(seg) + "] or beyond haystack_len";
}

}  // namespace acgpu_capi

namespace {

constexpr size_t kListHead = kBatchListHead;

acgpu_status bad_argument(const std::string& why) {
    g_last_error = "acgpu_find_batch: " + why;
    return ACGPU_ERR_INVALID_ARGUMENT;
}

acgpu_status bad_offsets(uint64_t seg) {
    return bad_argument(batch_bad_offsets_text(seg));
}

}  // namespace

acgpu_status acgpu_batch_plan_of(acgpu_automaton* aut, uint32_t* form) {
    if (!aut || !form) return ACGPU_ERR_INVALID_ARGUMENT;
    DeviceState* ds = nullptr;
    if (acgpu_status st = get_device_state(aut, &ds)) return st;
    *form = uint32_t(plan_batch(batch_facts(ds)));
    return ACGPU_OK;
}

extern "C" acgpu_status acgpu_find_batch(acgpu_automaton* aut, const acgpu_input* in, const uint64_t* offsets, size_t n,
                                         acgpu_match* out, acgpu_profile* prof) {
    // ---- checks, all before any device work
    if (!aut) return bad_argument("aut is NULL");
    if (!in) return bad_argument("in is NULL");
    if (prof) std::memset(prof, 0, sizeof *prof);
    if (n == 0) return ACGPU_OK;
    if (!offsets) return bad_argument("offsets is NULL");
    if (!out) return bad_argument("out is NULL");
    acgpu_input whole = *in;   // (the offsets are the spans)
    whole.span_start = 0; whole.span_end = in->haystack_len;
    acgpu_status st = check_nonoverlapping(aut, &whole);
    if (st) return st;
    const uint32_t lane_max = aut->var.batch_lane_max > 0 ? uint32_t(aut->var.batch_lane_max) : kBatchLaneMaxDefault;
    // an upper bound of the long segments: counted where the offsets are the host's, else what the haystack has room for
    uint64_t max_long = std::min<uint64_t>(n, in->haystack_len / (uint64_t(lane_max) + 1));
    if (!in->haystack_on_device) {   // host offsets: refused here; device offsets: by the classify kernel, same message
        max_long = 0;
        for (size_t s = 0; s < n; s++) {
            if (offsets[s + 1] < offsets[s] || offsets[s + 1] > in->haystack_len) return bad_offsets(s);
            max_long += offsets[s + 1] - offsets[s] > lane_max;
        }
    }

    // ---- device inputs
    DeviceState* ds = nullptr;
    if ((st = get_device_state(aut, &ds))) return st;
    ScratchLease lease(ds);
    Scratch* sc = lease.s.get();
    hipStream_t stream = static_cast<hipStream_t>(in->stream);
    if (prof && (st = ensure_events(sc))) return st;
    const uint64_t* doff = offsets;
    size_t lo = 0, hi = in->haystack_len;
    if (!in->haystack_on_device) {
        lo = offsets[0]; hi = offsets[n];
        HIP_TRY(sc->boff.ensure((n + 1) * sizeof(uint64_t)));
        HIP_TRY(hipMemcpyAsync(sc->boff.p, offsets, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
        doff = sc->boff.as<uint64_t>();
    }
    const uint8_t* dhay = nullptr;
    if ((st = device_haystack(in, lo, hi, sc, stream, &dhay))) return st;
    if (!in->out_on_device) HIP_TRY(sc->bout.ensure(n * sizeof(acgpu_match)));
    acgpu_match* dout = in->out_on_device ? out : sc->bout.as<acgpu_match>();
    HIP_TRY(sc->blongs.ensure(n * sizeof(BatchLong)));
    HIP_TRY(sc->bctl.ensure(kBatchCtlWords * sizeof(uint64_t)));
    const size_t pin_words = kBatchCtlWords + 3 * kListHead;
    if (!sc->bpin) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&sc->bpin), pin_words * sizeof(uint64_t)));

    BatchArgs a{};
    a.mis = uint64_t(reinterpret_cast<uintptr_t>(dhay) & 15);
    a.hay16 = dhay - a.mis;
    a.hay_len = in->haystack_len;
    a.off = doff; a.n_seg = n; a.out = dout;
    a.ctl = sc->bctl.as<unsigned long long>();
    a.longs = sc->blongs.as<BatchLong>(); a.longs_cap = n;
    a.lane_max = lane_max;
    a.anchored = in->anchored != 0;
    a.earliest = in->earliest != 0 || aut->cfg.match_kind == ACGPU_MATCH_STANDARD;   // src/automaton.rs:1259-1275
#ifdef ACGPU_GUARD
    a.guard = guard_counter();
    a.guard_lo = (lo + a.mis) & ~uint64_t(15);
    a.guard_hi = (hi + a.mis + 15) & ~uint64_t(15);
#endif
    const BatchForm form = plan_batch(batch_facts(ds));
    BatchRows rows{};
    if (form == BatchForm::LdsRows) rows = batch_rows_of(ds);

    // ---- the long segments: on the device (the scout walks the Standard automaton of the patterns: this one, or its twin), or
    // by the host after the synchronisation; a call that cannot have any queues nothing for them
    const BatchLongForm long_form = plan_batch_long(batch_long_facts(aut, in, lane_max));
    const bool on_device = long_form != BatchLongForm::HostCalls;
    BatchLongArgs la{};
    DeviceState* ods = ds;
    if (on_device && max_long) {
        la.max_len = uint32_t(aut->nnfa.max_pattern_len);
        la.scouted = long_form == BatchLongForm::ScoutResolve;
        la.leftmost = !a.earliest;
        if (la.scouted) {
            if (aut->occ && (st = get_device_state(aut->occ.get(), &ods))) return st;
            la.window = batch_long_window(aut->nnfa.max_pattern_len);
            HIP_TRY(sc->blkey.ensure(n * sizeof(uint64_t)));
            HIP_TRY(sc->bwpre.ensure((n + 1) * sizeof(uint64_t)));
            a.lkey = sc->blkey.as<unsigned long long>();
            la.wpre = sc->bwpre.as<uint64_t>();
        }
    }

    // ---- classify -> walk -> (scan -> scout -> resolve) -> the control words, the head of the long list where the host
    // serves it, and (host output) the records: one synchronisation
    const uint32_t blocks = uint32_t(std::max(ds->var.batch_blocks, 0));
    if (prof) HIP_TRY(hipEventRecord(sc->ev[0], stream));
    HIP_TRY(launch_batch_classify(a, stream));
    if (prof) HIP_TRY(hipEventRecord(sc->ev[1], stream));
    HIP_TRY(launch_batch_find(uint32_t(form), ds->da, rows, a, blocks, stream));
    if (prof) HIP_TRY(hipEventRecord(sc->ev[2], stream));
    if (on_device && max_long) {
        if (la.scouted) {
            const BatchForm oform = plan_batch(batch_facts(ods));
            const BatchRows orows = oform == BatchForm::LdsRows ? batch_rows_of(ods) : BatchRows{};
            const uint64_t max_windows = (hi - lo) / la.window + max_long;
            HIP_TRY(launch_batch_long_scan(a, la, stream));
            HIP_TRY(launch_batch_scout(uint32_t(oform), ods->da, orows, a, la, max_windows, blocks, stream));
        }
        HIP_TRY(launch_batch_resolve(ds->da, a, la, max_long, stream));
    }
    if (prof) HIP_TRY(hipEventRecord(sc->ev[3], stream));
    const size_t head = on_device ? 0 : std::min(n, kListHead);
    HIP_TRY(hipMemcpyAsync(sc->bpin, a.ctl, kBatchCtlWords * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    if (head) HIP_TRY(hipMemcpyAsync(sc->bpin + kBatchCtlWords, a.longs, head * sizeof(BatchLong), hipMemcpyDeviceToHost, stream));
    if (!in->out_on_device) HIP_TRY(hipMemcpyAsync(out, dout, n * sizeof(acgpu_match), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const uint64_t bad = sc->bpin[0], n_long = sc->bpin[1];
    uint64_t n_found = sc->bpin[2];
    if (bad != ~uint64_t(0)) return bad_offsets(bad);
    if (n_long > n || (on_device && n_long > max_long)) return ACGPU_ERR_HIP;

    // ---- the long segments the device did not serve: acgpu_find on their span (the haystack is on the device by now)
    const uint64_t n_host = on_device ? 0 : n_long;
    std::vector<BatchLong> longs(n_host);
    std::memcpy(longs.data(), sc->bpin + kBatchCtlWords, std::min<size_t>(n_host, head) * sizeof(BatchLong));
    if (n_host > head) HIP_TRY(hipMemcpy(longs.data() + head, a.longs + head, (n_host - head) * sizeof(BatchLong), hipMemcpyDeviceToHost));
    std::vector<acgpu_match> found_long(n_host);
    for (size_t i = 0; i < n_host; i++) {
        acgpu_input li = *in;
        li.haystack = dhay; li.haystack_on_device = 1; li.out_on_device = 0;
        li.span_start = size_t(longs[i].begin); li.span_end = size_t(longs[i].end);
        int32_t found = 0;
        acgpu_match m{};
        if ((st = acgpu_find(aut, &li, &found, &m))) return st;
        if (!found) { m = acgpu_match{}; m.pattern = ACGPU_NO_MATCH; }
        m._pad = 0;
        n_found += found ? 1 : 0;
        found_long[i] = m;
        if (in->out_on_device) HIP_TRY(hipMemcpyAsync(out + longs[i].seg, &found_long[i], sizeof m, hipMemcpyHostToDevice, stream));
        else out[longs[i].seg] = m;
    }
    if (n_host && in->out_on_device) HIP_TRY(hipStreamSynchronize(stream));

    if (prof) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, sc->ev[0], sc->ev[1])); prof->ms_compact = ms;   // control words + classification
        HIP_TRY(hipEventElapsedTime(&ms, sc->ev[1], sc->ev[2])); prof->ms_scan = ms;
        HIP_TRY(hipEventElapsedTime(&ms, sc->ev[2], sc->ev[3])); prof->ms_fill = ms;     // long segments on the device: scan, scout, resolve
        HIP_TRY(hipEventElapsedTime(&ms, sc->ev[0], sc->ev[3])); prof->ms_total = ms;
        prof->bytes_scanned = hi - lo;
        prof->n_chunks = (n + 63) / 64;       // wave tasks
        prof->n_active_chunks = n_long;       // segments longer than a lane walks ...
        prof->routed = uint32_t(std::min<uint64_t>(n_host, UINT32_MAX));   // ... and those of them that acgpu_find served
        prof->n_matches = n_found;
        prof->engine_used = uint32_t(form);   // (BatchForm is numbered as acgpu_engine)
    }
    return ACGPU_OK;
}

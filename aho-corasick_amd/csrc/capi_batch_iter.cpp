// C ABI of libacgpu.so, batched iterator (acgpu_find_iter_batch): every match of every segment of a packed haystack, CSR
// output, one call for millions of short texts.  control words + classify (device/batch_find.hip) -> count
// (device/batch_iter.hip) -> scan (launch_scan) -> SYNCHRONISATION 1: the offsets' error flag, the total, the list of the
// segments too long for a lane -> capacity check -> fill -> result copies -> SYNCHRONISATION 2.  The long segments of an
// overlapping call are served on the device where plan_batch_iter_long says so (device/batch_iter_long.hip): window-count scan,
// count and prefix in front of the scan -- which then covers short and long segments alike --, their fill behind the fill;
// two synchronisations however many there are.  Otherwise they are served between the two by acgpu_find_iter /
// acgpu_find_overlapping on their span: their counts are patched on the device, the scan runs again, and their records are
// put at rec_off[seg] behind the fill.  See capi_batch.cpp.
#include "capi_impl.hpp"

using namespace acgpu;
using namespace acgpu_capi;

namespace acgpu_capi {
#ifdef ACGPU_GUARD
unsigned long long* guard_counter();   // capi.cpp
#endif
}  // namespace acgpu_capi

namespace {

acgpu_status bad_argument(const std::string& why) {
    g_last_error = "acgpu_find_iter_batch: " + why;
    return ACGPU_ERR_INVALID_ARGUMENT;
}

// every record of one long span, by the single-span call
acgpu_status long_records(acgpu_automaton* aut, const acgpu_input* li, bool overlapping, std::vector<acgpu_match>* recs) {
    size_t cap = 4096, m = 0;
    for (;;) {
        recs->resize(cap);
        const acgpu_status st = overlapping ? acgpu_find_overlapping(aut, li, recs->data(), cap, &m) : acgpu_find_iter(aut, li, recs->data(), cap, &m);
        if (st == ACGPU_ERR_BUFFER_TOO_SMALL && m > cap) { cap = m; continue; }
        if (st) return st;
        recs->resize(m);
        for (auto& r : *recs) r._pad = 0;
        return ACGPU_OK;
    }
}

}  // namespace

extern "C" acgpu_status acgpu_find_iter_batch(acgpu_automaton* aut, const acgpu_input* in, const uint64_t* offsets, size_t n,
                                              int overlapping, uint64_t* rec_offsets, acgpu_match* out, size_t cap, size_t* n_out,
                                              acgpu_profile* prof) {
    // ---- checks, all before any device work
    if (!aut) return bad_argument("aut is NULL");
    if (!in) return bad_argument("in is NULL");
    if (!n_out) return bad_argument("n_out is NULL");
    *n_out = 0;
    if (prof) std::memset(prof, 0, sizeof *prof);
    if (n == 0) {
        if (rec_offsets && !in->out_on_device) rec_offsets[0] = 0;
        return ACGPU_OK;
    }
    if (!offsets) return bad_argument("offsets is NULL");
    if (!rec_offsets) return bad_argument("rec_offsets is NULL");
    if (!out && cap) return bad_argument("out is NULL");
    acgpu_input whole = *in;   // (the offsets are the spans)
    whole.span_start = 0; whole.span_end = in->haystack_len;
    acgpu_automaton* twin = nullptr;   // (not used: every stepper walks the automaton's own tables)
    acgpu_status st = overlapping ? check_overlapping(aut, &whole, &twin) : check_nonoverlapping(aut, &whole);
    if (st) return st;
    const uint32_t lane_max = aut->var.batch_lane_max > 0 ? uint32_t(aut->var.batch_lane_max) : kBatchLaneMaxDefault;
    // an upper bound of the long segments: counted where the offsets are the host's, else what the haystack has room for
    uint64_t max_long = std::min<uint64_t>(n, in->haystack_len / (uint64_t(lane_max) + 1));
    if (!in->haystack_on_device) {   // host offsets: refused here; device offsets: by the classify kernel, same message
        max_long = 0;
        for (size_t s = 0; s < n; s++) {
            if (offsets[s + 1] < offsets[s] || offsets[s + 1] > in->haystack_len) return bad_argument(batch_bad_offsets_text(s));
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
    HIP_TRY(sc->offsets.ensure((n + 1) * sizeof(uint64_t)));
    ScanScratch ss;
    if ((st = scan_scratch(sc, n, true, &ss))) return st;
    uint64_t* drec = in->out_on_device ? rec_offsets : sc->offsets.as<uint64_t>();
    ss.offsets = drec;
    HIP_TRY(sc->ensure_pinned());
    ss.host_totals = sc->pinned;   // the scan reports the total there
    HIP_TRY(sc->blongs.ensure(n * sizeof(BatchLong)));
    HIP_TRY(sc->bctl.ensure(kBatchCtlWords * sizeof(uint64_t)));
    const size_t pin_words = kBatchCtlWords + 3 * kBatchListHead;
    if (!sc->bpin) HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&sc->bpin), pin_words * sizeof(uint64_t)));

    BatchIterArgs ia{};
    BatchArgs& a = ia.b;
    a.mis = uint64_t(reinterpret_cast<uintptr_t>(dhay) & 15);
    a.hay16 = dhay - a.mis;
    a.hay_len = in->haystack_len;
    a.off = doff; a.n_seg = n; a.out = nullptr;
    a.ctl = sc->bctl.as<unsigned long long>();
    a.longs = sc->blongs.as<BatchLong>(); a.longs_cap = n;
    a.lane_max = lane_max;
    a.anchored = in->anchored != 0;
    a.earliest = in->earliest != 0 || aut->cfg.match_kind == ACGPU_MATCH_STANDARD;   // FindIter keeps the caller's flag (automaton.rs:864-883)
#ifdef ACGPU_GUARD
    a.guard = guard_counter();
    a.guard_lo = (lo + a.mis) & ~uint64_t(15);
    a.guard_hi = (hi + a.mis + 15) & ~uint64_t(15);
#endif
    ia.counts = ss.counts; ia.rec_off = drec; ia.overlapping = overlapping != 0;
    const BatchForm form = plan_batch_iter(batch_facts(ds));
    BatchIterRows rows{};
    if (form == BatchForm::LdsRows) {
        const BatchTables& t = ds->batch;
        rows.r.rows = t.rows.as<uint16_t>(); rows.r.first = t.first.as<uint32_t>(); rows.r.classes = ds->da.dfa.classes;
        rows.r.rows_bytes = t.rows_bytes; rows.r.alphabet_len = t.alphabet_len;
        rows.r.start_unanchored = t.start_unanchored; rows.r.start_anchored = t.start_anchored;
        rows.r.max_special = t.max_special; rows.r.max_match = t.max_match;
        rows.list_off = t.list_off.as<uint32_t>(); rows.list = t.list.as<uint32_t>();
    }
    const uint32_t blocks = uint32_t(std::max(ds->var.batch_blocks, 0));

    // ---- the long segments: on the device, or by the host after synchronisation 1; a call that cannot have any queues
    // nothing for them.  Scratch is sized by what the host knows now: a segment of k bytes has ceil(k / window) windows
    const bool on_device = plan_batch_iter_long(batch_long_facts(aut, in, lane_max), overlapping != 0) == BatchIterLongForm::WindowWalk;
    const bool dev_long = on_device && max_long > 0;
    BatchLongArgs la{};
    BatchIterLongArgs ila{};
    if (dev_long) {
        la.max_len = uint32_t(aut->nnfa.max_pattern_len);
        la.window = batch_long_window(aut->nnfa.max_pattern_len);
        ila.cap_windows = (hi - lo) / la.window + max_long;
        HIP_TRY(sc->bwpre.ensure((n + 1) * sizeof(uint64_t)));
        HIP_TRY(sc->bilane.ensure(ila.cap_windows * 64 * sizeof(uint32_t)));
        HIP_TRY(sc->biwsum.ensure(ila.cap_windows * sizeof(uint64_t)));
        la.wpre = sc->bwpre.as<uint64_t>();
        ila.lane_cnt = sc->bilane.as<uint32_t>();
        ila.wsum = sc->biwsum.as<uint64_t>();
    }

    // ---- classify -> count -> (window-count scan -> count -> prefix of the long segments) -> scan -> the control words, the
    // total and, where the host serves them, the head of the long list: synchronisation 1
    if (prof) HIP_TRY(hipEventRecord(sc->ev[0], stream));
    HIP_TRY(launch_batch_classify(a, stream));
    HIP_TRY(launch_batch_iter_count(uint32_t(form), ds->da, rows, ia, blocks, stream));
    if (dev_long) {
        if (prof) HIP_TRY(hipEventRecord(sc->ev[4], stream));
        HIP_TRY(launch_batch_long_scan(a, la, stream));
        HIP_TRY(launch_batch_iter_long_count(uint32_t(form), ds->da, rows, ia, la, ila, blocks, stream));
        HIP_TRY(launch_batch_iter_long_prefix(ia, la, ila, max_long, stream));
        if (prof) HIP_TRY(hipEventRecord(sc->ev[5], stream));
    }
    HIP_TRY(launch_scan(ss, n, stream));
    HIP_TRY(launch_batch_iter_seal(ss.totals, drec + n, stream));
    if (prof) HIP_TRY(hipEventRecord(sc->ev[1], stream));
    const size_t head = on_device ? 0 : std::min<size_t>(n, kBatchListHead);
    HIP_TRY(hipMemcpyAsync(sc->bpin, a.ctl, kBatchCtlWords * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    if (head) HIP_TRY(hipMemcpyAsync(sc->bpin + kBatchCtlWords, a.longs, head * sizeof(BatchLong), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const uint64_t bad = sc->bpin[0], n_all_long = sc->bpin[1];
    if (bad != ~uint64_t(0)) return bad_argument(batch_bad_offsets_text(bad));
    if (n_all_long > n || (on_device && n_all_long > max_long)) return ACGPU_ERR_HIP;
    if (dev_long && sc->bpin[2]) return bad_argument("a segment has 2^32 records or more");   // (control word [2]: the prefix kernel's)
    uint64_t total = sc->pinned[0];

    // ---- the long segments the device did not serve: the single-span call on each (the haystack is on the device by now),
    // their counts patched on the device, the scan again
    const uint64_t n_long = on_device ? 0 : n_all_long;
    std::vector<BatchLong> longs(n_long);
    std::vector<std::vector<acgpu_match>> long_recs(n_long);
    std::vector<uint32_t> long_counts(n_long);
    std::vector<uint64_t> long_at(n_long);
    if (n_long) {
        std::memcpy(longs.data(), sc->bpin + kBatchCtlWords, std::min<size_t>(n_long, head) * sizeof(BatchLong));
        if (n_long > head) HIP_TRY(hipMemcpy(longs.data() + head, a.longs + head, (n_long - head) * sizeof(BatchLong), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n_long; i++) {
            acgpu_input li = *in;
            li.haystack = dhay; li.haystack_on_device = 1; li.out_on_device = 0;
            li.span_start = size_t(longs[i].begin); li.span_end = size_t(longs[i].end);
            if ((st = long_records(aut, &li, overlapping != 0, &long_recs[i]))) return st;
            if (long_recs[i].size() > UINT32_MAX) return bad_argument("a segment has 2^32 records or more");
            long_counts[i] = uint32_t(long_recs[i].size());
            HIP_TRY(hipMemcpyAsync(ss.counts + longs[i].seg, &long_counts[i], sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        }
        HIP_TRY(launch_scan(ss, n, stream));
        HIP_TRY(launch_batch_iter_seal(ss.totals, drec + n, stream));
        for (size_t i = 0; i < n_long; i++)
            HIP_TRY(hipMemcpyAsync(&long_at[i], drec + longs[i].seg, sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        total = sc->pinned[0];
    }

    if (prof) {
        prof->bytes_scanned = hi - lo;
        prof->n_chunks = (n + 63) / 64;       // wave tasks
        prof->n_active_chunks = n_all_long;   // segments longer than a lane walks ...
        prof->routed = uint32_t(std::min<uint64_t>(n_long, UINT32_MAX));   // ... and those of them that the single-span calls served
        prof->n_matches = total;
        prof->engine_used = uint32_t(form);   // (BatchForm is numbered as acgpu_engine)
    }
    *n_out = size_t(total);
    if (total > cap) {   // (nothing written to `out`)
        if (prof) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, sc->ev[0], sc->ev[1])); prof->ms_compact = ms; prof->ms_total = ms;
            if (dev_long) { HIP_TRY(hipEventElapsedTime(&ms, sc->ev[4], sc->ev[5])); prof->ms_fill = ms; }
        }
        return ACGPU_ERR_BUFFER_TOO_SMALL;
    }

    // ---- fill -> the long segments' records -> (host output) the result copies: synchronisation 2
    if (!in->out_on_device) HIP_TRY(sc->bout.ensure(std::max<size_t>(total, 1) * sizeof(acgpu_match)));
    acgpu_match* dout = in->out_on_device ? out : sc->bout.as<acgpu_match>();
    a.out = dout;
    if (prof) HIP_TRY(hipEventRecord(sc->ev[2], stream));
    if (total) HIP_TRY(launch_batch_iter_fill(uint32_t(form), ds->da, rows, ia, blocks, stream));
    if (prof) HIP_TRY(hipEventRecord(sc->ev[3], stream));
    if (dev_long) {   // (behind the fill: a staged task of k_batch_iter stores its whole range, a long segment's part included)
        if (total) HIP_TRY(launch_batch_iter_long_fill(uint32_t(form), ds->da, rows, ia, la, ila, blocks, stream));
        if (prof) HIP_TRY(hipEventRecord(sc->ev[6], stream));
    }
    for (size_t i = 0; i < n_long; i++)
        if (long_counts[i])
            HIP_TRY(hipMemcpyAsync(dout + long_at[i], long_recs[i].data(), long_counts[i] * sizeof(acgpu_match), hipMemcpyHostToDevice, stream));
    if (!in->out_on_device) {
        HIP_TRY(hipMemcpyAsync(rec_offsets, drec, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        if (total) HIP_TRY(hipMemcpyAsync(out, dout, total * sizeof(acgpu_match), hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));

    if (prof) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, sc->ev[0], sc->ev[1])); prof->ms_compact = ms;   // classification + count + scan
        HIP_TRY(hipEventElapsedTime(&ms, sc->ev[2], sc->ev[3])); prof->ms_scan = ms;      // fill
        HIP_TRY(hipEventElapsedTime(&ms, sc->ev[0], sc->ev[dev_long ? 6 : 3])); prof->ms_total = ms;
        if (dev_long) {   // the long segments on the device: window-count scan + count + prefix (inside ms_compact), and their fill
            float ms_fill = 0;
            HIP_TRY(hipEventElapsedTime(&ms, sc->ev[4], sc->ev[5]));
            HIP_TRY(hipEventElapsedTime(&ms_fill, sc->ev[3], sc->ev[6]));
            prof->ms_fill = ms + ms_fill;
        }
    }
    return ACGPU_OK;
}

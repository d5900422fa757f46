// Builder of the batched find's LDS image (batch_tables.hpp).
#include "batch_tables.hpp"

#include "engine_plan.hpp"

namespace acgpu {

bool build_batch_image(const Dfa& d, const std::vector<uint32_t>& pattern_lens, BatchImage& out) {
    const uint32_t alen = uint32_t(d.alphabet_len);
    if (!batch_rows_fit(d.state_len, alen) || d.trans.size() < (d.state_len << d.stride2)) return false;
    BatchImage img;
    img.alphabet_len = alen;
    auto off_of = [&](uint32_t sid) { return (sid >> d.stride2) * alen; };   // (< 65 536: batch_rows_fit)
    const size_t entries = d.state_len * alen;
    img.rows.assign((entries + 7) & ~size_t(7), 0);
    for (size_t i = 0; i < d.state_len; i++)
        for (uint32_t c = 0; c < alen; c++) {
            const uint32_t next = d.trans[(i << d.stride2) + c];
            if ((next >> d.stride2) >= d.state_len) return false;
            img.rows[i * alen + c] = uint16_t(off_of(next));
        }
    img.first.assign(2 * d.num_match_states, 0);
    img.list_off.assign(2 * d.num_match_states, 0);
    for (size_t m = 0; m < d.num_match_states; m++) {
        if (d.moff[m + 1] == d.moff[m]) return false;   // (a match state reports at least one pattern)
        const uint32_t pid = d.mpid[d.moff[m]];
        if (pid >= pattern_lens.size()) return false;
        img.first[2 * m] = pid;
        img.first[2 * m + 1] = pattern_lens[pid];
        img.list_off[2 * m] = uint32_t(img.list.size() / 2);
        img.list_off[2 * m + 1] = d.moff[m + 1] - d.moff[m];
        for (uint32_t i = d.moff[m]; i < d.moff[m + 1]; i++) {
            if (d.mpid[i] >= pattern_lens.size()) return false;
            img.list.push_back(d.mpid[i]);
            img.list.push_back(pattern_lens[d.mpid[i]]);
        }
    }
    img.start_unanchored = off_of(d.special.start_unanchored_id);
    img.start_anchored = off_of(d.special.start_anchored_id);
    img.max_special = off_of(d.special.max_special_id);
    img.max_match = off_of(d.special.max_match_id);
    out = std::move(img);
    return true;
}

hipError_t upload_batch_tables(const Dfa& d, const std::vector<uint32_t>& pattern_lens, bool want_rows, BatchTables& out) {
    out.ready = false;
    out.dfa_states = d.state_len;
    out.alphabet_len = uint32_t(d.alphabet_len);
    BatchImage img;
    if (!want_rows || !build_batch_image(d, pattern_lens, img)) return hipSuccess;
    if (hipError_t e = out.rows.upload(img.rows); e != hipSuccess) return e;
    if (hipError_t e = out.first.upload(img.first); e != hipSuccess) return e;
    if (hipError_t e = out.list_off.upload(img.list_off); e != hipSuccess) return e;
    if (hipError_t e = out.list.upload(img.list); e != hipSuccess) return e;
    out.rows_bytes = uint32_t(img.rows.size() * sizeof(uint16_t));
    out.start_unanchored = img.start_unanchored; out.start_anchored = img.start_anchored;
    out.max_special = img.max_special; out.max_match = img.max_match;
    out.ready = true;
    return hipSuccess;
}

}  // namespace acgpu

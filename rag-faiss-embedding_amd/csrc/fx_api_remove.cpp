// fx_api_remove.cpp -- remove_ids (fx_remove.hip): the compaction of the stored rows under a selector.
#include "fx_host.h"
#include "fx_plan.h"

using namespace fx;

namespace {

// The compaction itself: the index's rows under sel's mask (sel->rows > 0 of
// them removed), then the invariants of grow() / fx_index_reset on the freed
// tail, the recomputed norm maximum and the scan image's bookkeeping.
int remove_rows(FxIndex* h, const FxSelector* sel) {
    hipStream_t s = h->stream();
    const int64_t nt = h->ntotal, rb = h->row_bytes;
    const int64_t nw = sel_mask_words(nt), ngp = rm_groups(nt), nblk = rm_prefix_blocks(nt);
    int64_t stage_bytes = h->opt.remove_stage;
    if (stage_bytes < rb || stage_bytes > REMOVE_STAGE_MAX) stage_bytes = REMOVE_STAGE_DEFAULT;
    const int64_t stage_rows = std::min(std::max<int64_t>(stage_bytes / rb, 1), nt);
    HIP_TRY(h->rm.ws.ensure((size_t)(nw + ngp + nblk + 4 + stage_rows) * 4));
    unsigned* prefix = (unsigned*)h->rm.ws.p;
    unsigned* gp = prefix + nw;
    unsigned* bsum = gp + ngp;
    unsigned* info = bsum + nblk;
    float* nstage = (float*)(info + 4);
    HIP_TRY(launch_keep_prefix(sel->mask, nt, prefix, gp, bsum, info, s));
    unsigned hinfo[2] = {0u, 0u};
    HIP_TRY(hipMemcpyAsync(hinfo, info, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    KeptPrefix P;
    P.ntotal = nt;
    P.first = hinfo[0];
    P.kept = hinfo[1];
    if (P.first >= nt || P.kept != nt - sel->rows)
        return set_err(FX_E_INTEGRITY, "remove_ids: the mask's scan gives first removed row %lld, %lld kept of %lld rows; "
                       "the selector counted %lld selected", (long long)P.first, (long long)P.kept, (long long)nt,
                       (long long)sel->rows);
    P.g = stage_rows < std::min<int64_t>(RM_GROUP_ROWS, nt) ? 1 : RM_GROUP_ROWS;
    if (P.g == 1) {
        P.words.resize((size_t)nw);
        P.mask.resize((size_t)nw);
        HIP_TRY(hipMemcpyAsync(P.words.data(), prefix, (size_t)nw * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(P.mask.data(), sel->mask, (size_t)nw * 4, hipMemcpyDeviceToHost, s));
    } else {
        P.gp.resize((size_t)ngp);
        HIP_TRY(hipMemcpyAsync(P.gp.data(), gp, (size_t)ngp * 4, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<RemoveChunk> plan;
    if (!plan_remove(P, stage_rows, plan)) return set_err(FX_E_INTEGRITY, "remove_ids: no chunk plan within the staging buffer");
    int64_t staged_max = 0;
    for (const RemoveChunk& c : plan)
        if (!c.direct) staged_max = std::max(staged_max, c.kept);
    if (staged_max > stage_rows) return set_err(FX_E_INTEGRITY, "remove_ids: a staged chunk exceeds the staging buffer");
    if (staged_max > 0) HIP_TRY(h->stage.ensure((size_t)staged_max * rb));
    h->rm.stats[0] = P.first;
    h->rm.stats[1] = h->rm.stats[2] = 0;
    h->rm.stats[3] = (int64_t)plan.size();
    for (const RemoveChunk& c : plan) h->rm.stats[c.direct ? 1 : 2] += c.kept;
    for (const RemoveChunk& c : plan) {
        if (c.direct) {
            HIP_TRY(launch_move_rows(h->codes, h->norms, sel->mask, prefix, nt, (int)rb, c.s0, c.s1, h->codes, h->norms, 0, s));
        } else {
            HIP_TRY(launch_move_rows(h->codes, h->norms, sel->mask, prefix, nt, (int)rb, c.s0, c.s1, (char*)h->stage.p,
                                     nstage, c.d0, s));
            HIP_TRY(hipMemcpyAsync(h->codes + (size_t)c.d0 * rb, h->stage.p, (size_t)c.kept * rb, hipMemcpyDeviceToDevice, s));
            HIP_TRY(hipMemcpyAsync(h->norms + c.d0, nstage, (size_t)c.kept * 4, hipMemcpyDeviceToDevice, s));
        }
    }
    const int64_t newn = P.kept;
    if (h->has_ids) {
        // the labels follow their rows: compacted out of place into the second buffer, which takes over
        // (searches enqueued before this call are done with the old one: the sync below precedes any reuse)
        if (h->idm.labels_alt.bytes < h->idm.labels.bytes) {
            h->idm.labels_alt.release();
            HIP_TRY(h->idm.labels_alt.ensure(h->idm.labels.bytes));
        }
        HIP_TRY(launch_compact_labels(h->idm.labels, sel->mask, prefix, nt, h->idm.labels_alt, s));
        h->idm.labels.swap(h->idm.labels_alt);
    }
    HIP_TRY(blank_rows(h, newn, nt, s));  // the freed tail
    // max |y|^2 over the kept rows (a removed outlier's would keep the certification bound E wide for good)
    HIP_TRY(hipMemsetAsync(h->max_sq_bits, 0, 4, s));
    HIP_TRY(launch_norm_max(h->norms, newn, h->max_sq_bits, s));
    // scan image: rows below the first removed one stay valid for the unchanged centre; update_scan_image
    // rebuilds the rest at the next search.  Its freed tail: +inf row constants, zero F32S rows.
    h->img_rows = std::min(h->img_rows, P.first);
    if (h->cnorms.p) {
        const int64_t hi = std::min<int64_t>(nt, (int64_t)(h->cnorms.bytes / 4));
        if (newn < hi)
            HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)((float*)h->cnorms.p + newn), 0x7f800000u, (size_t)(hi - newn), s));
        if (h->img_kind != IMG_NONE) {  // ... and its maximum over the rows that stay
            HIP_TRY(hipMemsetAsync(h->max_sq_bits + 1, 0, 4, s));
            HIP_TRY(launch_norm_max((const float*)h->cnorms.p, std::min<int64_t>(h->img_rows, hi), h->max_sq_bits + 1, s));
        }
    }
    if (h->split.p) {
        const int64_t hi = std::min<int64_t>(nt, (int64_t)(h->split.bytes / rb));
        if (newn < hi) HIP_TRY(hipMemsetAsync((char*)h->split.p + (size_t)newn * rb, 0, (size_t)(hi - newn) * rb, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    h->ntotal = newn;
    if (newn == 0) h->mu_rows = 0;  // as fx_index_reset leaves it
    ++h->epoch;
    h->rg.nq = -1;  // the last range search's result named the old rows
    h->rg.total = 0;
    graph_release(h);  // (its key would not notice a removal followed by an add of as many rows)
    return FX_OK;
}

}  // namespace

extern "C" {

int fx_index_remove_ids(FxIndex* h, const FxSelector* sel, int64_t* n_removed) {
    if (!h) return set_err(FX_E_ARG, "null index");
    if (!sel) return set_err(FX_E_ARG, "null selector");
    if (!n_removed) return set_err(FX_E_ARG, "null n_removed");
    *n_removed = 0;
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = check_selector(h, sel, "remove_ids", "rows were added or removed, or the index was reset");
        rc != FX_OK)
        return rc;
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    {
        const int rc = selector_counts(sel);
        if (rc != FX_OK) return rc;
    }
    if (h->ntotal == 0 || sel->rows == 0) return FX_OK;  // nothing selected: nothing changes, the selector stays valid
    const int rc = remove_rows(h, sel);
    if (rc != FX_OK) return rc;
    *n_removed = sel->rows;
    return FX_OK;
}

int fx_index_last_remove_stats(FxIndex* h, int64_t* first, int64_t* direct_rows, int64_t* staged_rows, int64_t* chunks) {
    if (!h || !first || !direct_rows || !staged_rows || !chunks) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *first = h->rm.stats[0];
    *direct_rows = h->rm.stats[1];
    *staged_rows = h->rm.stats[2];
    *chunks = h->rm.stats[3];
    return FX_OK;
}

}  // extern "C"

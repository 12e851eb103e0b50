// fx_flat_codes.h -- the search of a flat index of codes (FlatCodes: FxSq, FxPq): one driver for the checks,
// the plan record, the staging, the pass loop with its events, the counts and the way back to a host caller.
// What differs between the two indexes is a traits type Ops of static functions over (H*, const CodePass&):
//   plan(h, nq, k) -> SqPlan             size(h, qb_max, pad_max): its query operands' workspace
//   prep / scan / refine / exact: one launch each            dump: the diagnostic build's FX_*_CAND record
#pragma once
#include "fx_plan.h"

namespace fx {

// one pass of a search: queries [q, q + nq) and their slice of the output
struct CodePass {
    const void* q;
    int q_dt, k;
    int64_t nq, nq_pad;
    const SqPlan* P;
    int* n_flag;  // device: the pass's flagged-query count
    float* D;
    int64_t* I;
    hipStream_t s;
};

template <class Ops, class H>
int flat_codes_search(H* h, const char* kind, int64_t nq, const void* q, int q_dtype, int q_mem, int k, float* D,
                      int64_t* I, int out_mem) {
    if (nq < 0) return set_err(FX_E_ARG, "negative nq");
    if (k < 1) return set_err(FX_E_ARG, "k must be positive (got %d)", k);
    if (!check_dtype(q_dtype)) return set_err(FX_E_ARG, "bad query dtype %d", q_dtype);
    if (!valid_mem(q_mem) || !valid_mem(out_mem)) return set_err(FX_E_ARG, "bad q_mem / out_mem");
    if (k > FX_MAX_K) return set_err(FX_E_UNSUPPORTED, "%s search: k = %d above FX_MAX_K = %d", kind, k, FX_MAX_K);
    if (!h) return set_err(FX_E_ARG, "null %s index", kind);
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = need_trained(h->trained, kind, "search"); rc != FX_OK) return rc;
    if (nq == 0) return FX_OK;
    if (!q || !D || !I) return set_err(FX_E_ARG, "null buffer");
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    hipStream_t s = h->stream();
    // (an earlier device search's counts, if nobody asked for them, give way to this search's)
    h->clear_counts();
    if (h->ntotal == 0) return fill_missing(s, h->metric, nq, k, D, I, out_mem);

    const SqPlan P = Ops::plan(h, nq, k);
    h->last_plan[0] = P.path;
    h->last_plan[1] = P.qtiles;
    h->last_plan[2] = P.splits;
    h->last_plan[3] = P.xsplits;
    h->last_qbatch = P.q_batch;
    h->last_grid = P.grid;
    const int qes = dtype_size(q_dtype);
    const void* qdev = nullptr;
    HIP_TRY(stage_in(s, h->in, q, (size_t)nq * h->d * qes, q_mem, &qdev));
    void *Dd = D, *Id = I;
    HIP_TRY(out_buf(h->outD, D, (size_t)nq * k * 4, out_mem, &Dd));
    HIP_TRY(out_buf(h->outI, I, (size_t)nq * k * 8, out_mem, &Id));
    const int64_t qb_max = std::min(P.q_batch, nq);
    HIP_TRY(Ops::size(h, qb_max, round_up(qb_max, QPAD)));
    HIP_TRY(h->eps.ensure((size_t)qb_max * 4));
    HIP_TRY(h->rho.ensure((size_t)qb_max * 4));
    HIP_TRY(h->shift.ensure((size_t)qb_max * 8));
    HIP_TRY(h->flag.ensure((size_t)(qb_max + 1) * 4));
    HIP_TRY(h->cand_d.ensure((size_t)P.cand_bytes / 2));
    HIP_TRY(h->cand_i.ensure((size_t)P.cand_bytes / 2));
    HIP_TRY(hipMemsetAsync(h->cnt, 0, 16, s));

    for (int64_t q0 = 0; q0 < nq; q0 += qb_max) {
        const int64_t qb = std::min(qb_max, nq - q0);
        const CodePass ps{(const char*)qdev + (size_t)q0 * h->d * qes, q_dtype, k, qb, round_up(qb, QPAD), &P,
                          (int*)h->flag.p, (float*)Dd + q0 * k, (int64_t*)Id + q0 * k, s};
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        HIP_TRY(h->begin_pass(ev, 4, s));
        // 1. query preparation: fp32 copies, the scan's operand planes, the bound's terms; n_flag <- 0
        HIP_TRY(Ops::prep(h, ps));
        HIP_TRY(h->mark(ev[1], s));
        if (P.path != SQ_PATH_FUSED) {
            // the exact path for the whole pass: every query "flagged"
            HIP_TRY(launch_ivf_flag_all(ps.n_flag, qb, s));
            HIP_TRY(Ops::exact(h, ps));
            HIP_TRY(h->mark(ev[2], s));  // (the exact scan is this path's "scan"; it has no refine)
            HIP_TRY(h->mark(ev[3], s));
            continue;
        }
        // 2. the MFMA scan: every (query tile, split) writes its sorted top-KP
        HIP_TRY(Ops::scan(h, ps));
        HIP_TRY(h->mark(ev[2], s));
#ifdef FX_DIAG
        // the pass's record, before the refine reads the lists and the exact scan writes over them
        if (const int rc = Ops::dump(h, ps); rc != FX_OK) return rc;
#endif
        // 3. refine + certification; every split pruned only with its own KP-th key
        HIP_TRY(Ops::refine(h, ps));
        // 4. the flagged queries' exact scan (device-gated; the candidate buffers are free again)
        HIP_TRY(Ops::exact(h, ps));
        HIP_TRY(launch_ivf_accum(h->cnt + 1, ps.n_flag, s));
        HIP_TRY(h->mark(ev[3], s));
    }
    HIP_TRY(hipMemcpyAsync(h->pin_cnt, h->cnt, 8, hipMemcpyDeviceToHost, s));
    h->counts_pending = true;
    if (out_mem != FX_MEM_HOST) return FX_OK;
    HIP_TRY(hipMemcpyAsync(D, Dd, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(I, Id, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s));
    if (const int rc = h->read_counts(h->device, s); rc != FX_OK) return rc;
    if (h->last_dropped > 0)
        return set_err(FX_E_INTEGRITY, "%s search: %lld candidate row ids outside [0, %lld) were dropped", kind,
                       (long long)h->last_dropped, (long long)h->ntotal);
    return FX_OK;
}

inline int flat_codes_last_plan(FlatCodes* h, int* path, int* qtiles, int* splits, int* xsplits, int64_t* q_batch,
                                int64_t* grid) {
    if (!h || !path || !qtiles || !splits || !xsplits || !q_batch || !grid) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *path = h->last_plan[0];
    *qtiles = h->last_plan[1];
    *splits = h->last_plan[2];
    *xsplits = h->last_plan[3];
    *q_batch = h->last_qbatch;
    *grid = h->last_grid;
    return FX_OK;
}

}  // namespace fx

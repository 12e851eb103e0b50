// fx_api_search.cpp -- search on the flat index: the scan image, the search plan (plan_search / plan_rescan)
// over the index's workspace, its enqueue, the host-output path, k > FX_BIG_K, the search graph,
// fx_index_search and the counters of the last search.
#include "fx_host.h"
#include "fx_plan.h"

using namespace fx;

namespace {

hipError_t ensure_pinned_count(FxIndex* h) {
    if (h->pin_nf) return hipSuccess;
    hipError_t e = h->pin_nf.ensure(3 * sizeof(int));
    if (e == hipSuccess) h->pin_nf[0] = h->pin_nf[1] = h->pin_nf[2] = 0;
    return e;
}

}  // namespace

// bring the scan image up to date (rows appended since the last search)
hipError_t fx::update_scan_image(FxIndex* h) {
    const int kind = image_kind(h->shape(), h->opt);
    hipStream_t s = h->stream();
    hipError_t e = hipSuccess;
    if (kind == IMG_NONE) {
        h->img_kind = IMG_NONE;
        return hipSuccess;
    }
    const void* old = h->split.p;
    const void* old_n = h->cnorms.p;
    if (kind == IMG_F32S && (e = h->split.ensure((size_t)h->cap_rows * h->row_bytes)) != hipSuccess) return e;
    if ((e = h->cnorms.ensure((size_t)h->cap_rows * 4)) != hipSuccess) return e;
    bool rebuild = h->split.p != old || h->cnorms.p != old_n || h->img_rows > h->ntotal || kind != h->img_kind;
    const bool centre = h->metric == L2 && h->opt.centre != 0;
    if (centre != h->centred) rebuild = true;
    if (centre && (h->mu_rows == 0 || h->ntotal >= 2 * h->mu_rows || kind != h->img_kind)) {
        // (re)centre on the current rows
        if ((e = h->centre.ensure((size_t)h->kdim * 4)) != hipSuccess) return e;
        if ((e = h->mu_part.ensure((size_t)2 * MU_GROUPS * h->kdim * 8)) != hipSuccess) return e;
        // 16-bit rows: a centre whose norm is below 0.1 of the rows' mean
        // square norm (no common direction) is dropped (mu = 0), which keeps
        // 16-bit-exact queries exact in the scan operand
        if ((e = launch_mu(h->codes, h->dtype, h->row_bytes, h->d, h->ntotal, (double*)h->mu_part.p,
                           (float*)h->centre.p, kind == IMG_C16 ? 0.1f : 0.0f, s)) != hipSuccess)
            return e;
        h->mu_rows = h->ntotal;
        rebuild = true;
    }
    h->centred = centre;
    h->img_kind = kind;
    if (rebuild) {  // zero image (finite padding rows), +inf padding norms
        if (kind == IMG_F32S && (e = hipMemsetAsync(h->split.p, 0, h->split.bytes, s)) != hipSuccess) return e;
        if ((e = hipMemsetD32Async((hipDeviceptr_t)h->cnorms.p, 0x7f800000u, h->cnorms.bytes / 4, s)) != hipSuccess)
            return e;
        if ((e = hipMemsetAsync(h->max_sq_bits + 1, 0, 4, s)) != hipSuccess) return e;
        h->img_rows = 0;
    }
    const float* mu = centre ? (const float*)h->centre.p : nullptr;
    if (kind == IMG_F32S)
        e = launch_split_rows((const float*)h->codes.p, h->kdim, h->img_rows, h->ntotal, mu, h->split.p,
                              (float*)h->cnorms.p, h->max_sq_bits + 1, s);
    else
        e = launch_centre_norms(h->codes, h->dtype, h->row_bytes, h->img_rows, h->ntotal, mu, (float*)h->cnorms.p,
                                h->max_sq_bits + 1, s);
    if (e == hipSuccess) h->img_rows = h->ntotal;
    return e;
}

void fx::base_prep(const FxIndex* h, const QueryBufs& b, const void* q, int q_dtype, int64_t nq, int64_t nq_pad,
                   int st_dt, PrepParams& pp) {
    pp.q = q;
    pp.q_dt = q_dtype;
    pp.nq = nq;
    pp.nq_pad = nq_pad;
    pp.d = h->d;
    pp.kdim = h->kdim;
    pp.st_dt = st_dt;
    pp.metric = h->metric;
    pp.qf32 = (float*)b.f32.p;
    pp.qop = b.op.p;
    pp.qeps = (float*)b.eps.p;
    pp.qrho = (float*)b.rho.p;
    pp.qshift = (double*)b.shift.p;
    pp.mbits = h->max_sq_bits;
    pp.img_bits = h->max_sq_bits;  // (a scan image has its own maximum: max_sq_bits + 1)
}

void fx::base_scan(const FxIndex* h, int img_kind, const QueryBufs& b, int64_t nq, ScanParams& sp) {
    sp.codes = img_kind == IMG_F32S ? (const char*)h->split.p : h->codes;
    sp.norms = img_kind != IMG_NONE ? (const float*)h->cnorms.p : h->norms;
    sp.ntotal = h->ntotal;
    sp.row_bytes = h->row_bytes;
    sp.qop = (const char*)b.op.p;
    sp.nq = nq;
}

namespace {

// the scan's plan for nq queries and k results: the filtered scan's with a selector (fx_plan.h)
void plan_index_scan(const FxIndex* h, bool sel, int64_t nq, int k, ScanParams& sp) {
    const IndexShape ix = h->shape();
    if (sel) plan_sel_scan(ix, nq, k, sp);
    else plan_scan(ix, h->opt, nq, k, scan_v5_qt(ix.img_kind == IMG_F32S ? (int)F32S : ix.dtype, ix.row_bytes), sp);
}

// The re-scan of the queries pass 1 could not certify (rows flag_list[0 ..
// n_flag) of the batch, gathered on the device): the same MFMA scan over
// them without cross-split pruning and with ~k1/4 corpus splits, then
// k_refine_big re-ranking k1 = max(512, 4k) approx candidates exactly, so the
// certification bound sits near the k1-th key instead of the ~2k-th.  Its
// uncertified queries go to the exact scan.  Launched always; every kernel
// reads the flagged count and exits at once when it is 0.
// The re-scan's workspace is sized for RESCAN_MAX flagged queries whatever
// the batch (its lists are k1/4 splits wide); a batch that could flag more
// runs it in ceil(nq / RESCAN_MAX) chunks over the flagged list, each chunk's
// live count decided on the device (k_rescan_chunks: empty chunks exit at
// once), so a large batch never pays for a workspace it almost never uses
// and never sends re-scannable queries to the exact scan.
hipError_t plan_rescan(FxIndex* h, SearchPlan& P) {
    hipError_t e;
    const int64_t nq = std::min<int64_t>(P.nq, RESCAN_MAX);
    const int k1 = std::min(2 * FX_BIG_K, std::max(512, 4 * P.k));
    int* n_flag = P.rp.n_flag;
    ScanParams& sp = P.sp2;
    sp = P.sp;
    sp.nq = nq;
    plan_index_scan(h, P.sel != nullptr, nq, k1, sp);  // k1 > KP: share = 0, >= k1/4 splits
    // (the convoy words hold CONV_MAX splits: pass 1's gate, taken again for this split count)
    sp.conv = sp.conv && sp.splits <= CONV_MAX ? sp.conv : nullptr;
    const int64_t nq_pad = round_up(nq, std::max<int64_t>(QPAD, sp.qt));
    if ((e = h->rq.f32.ensure((size_t)nq_pad * h->kdim * 4)) != hipSuccess) return e;
    if ((e = h->rq.op.ensure((size_t)nq_pad * h->row_bytes)) != hipSuccess) return e;
    if ((e = h->rq.eps.ensure((size_t)nq * 4)) != hipSuccess) return e;
    if ((e = h->rq.rho.ensure((size_t)nq * 4)) != hipSuccess) return e;
    if ((e = h->rq.shift.ensure((size_t)nq * 8)) != hipSuccess) return e;
    if ((e = h->rq.gtau.ensure((size_t)nq_pad * 4)) != hipSuccess) return e;
    P.nchunks = (int)((P.nq + RESCAN_MAX - 1) / RESCAN_MAX);
    // [count | every query may go exact | the chunks' live counts]
    if ((e = h->rq.flag.ensure((size_t)(P.nq + 1 + P.nchunks) * 4)) != hipSuccess) return e;
    PrepParams& pp = P.pp2;
    pp = P.pp;
    pp.nq = nq;
    pp.nq_pad = nq_pad;
    pp.q = h->qw.f32.p;  // pass 1's fp32 copy of the batch, rows padded to kdim
    pp.q_dt = F32;
    pp.d = h->kdim;
    pp.qidx = P.rp.flag_list;
    pp.nq_dev = n_flag;
    pp.qf32 = (float*)h->rq.f32.p;
    pp.qop = h->rq.op.p;
    pp.qeps = (float*)h->rq.eps.p;
    pp.qrho = (float*)h->rq.rho.p;
    pp.qshift = (double*)h->rq.shift.p;
    sp.qop = (const char*)h->rq.op.p;
    sp.gtau = (unsigned*)h->rq.gtau.p;
    sp.pub = nullptr;
    sp.prune_rank = KP;
    sp.dbg = 0;
    sp.trace = nullptr;
    sp.dbgbuf = nullptr;
    sp.stamps = nullptr;
    sp.nq_dev = n_flag;
    const size_t ncand = (size_t)sp.n_qtiles * sp.splits * sp.qt * KP;
    if ((e = h->rq.cand_d.ensure(ncand * 4)) != hipSuccess) return e;
    if ((e = h->rq.cand_i.ensure(ncand * 4)) != hipSuccess) return e;
    sp.cand_d = (float*)h->rq.cand_d.p;
    sp.cand_i = (int*)h->rq.cand_i.p;
    RefineParams& rp = P.rp2;
    rp = P.rp;
    rp.nq = nq;
    rp.cand_d = sp.cand_d;
    rp.cand_i = sp.cand_i;
    rp.splits = sp.splits;
    rp.qt = sp.qt;
    rp.qf32 = pp.qf32;
    rp.qeps = pp.qeps;
    rp.qrho = pp.qrho;
    rp.qshift = pp.qshift;
    rp.k1 = k1;
    rp.gtau = nullptr;
    rp.nq_dev = n_flag;
    rp.out_idx = P.rp.flag_list;
    P.n_exact = (int*)h->rq.flag.p;
    P.chunk_cnt = P.n_exact + 1 + P.nq;
    rp.n_flag = P.n_exact;
    rp.flag_list = P.n_exact + 1;
    rp.force_fb = h->opt.force_fallback == 2;
    rp.wg = 0;
    return hipSuccess;
}

// words (non-null: a host-output search): [n_drop | n_flag | flag list[nq]]
// inside the packed output buffer; otherwise the index's own counter words
hipError_t plan_search(FxIndex* h, int64_t nq, const void* qdev, int q_dtype, int k, float* Dd, int64_t* Id,
                       int* words, SearchPlan& P) {
    hipError_t e;
    P.nq = nq;
    P.k = k;
    P.q_dtype = q_dtype;
    // a filtered search scans the stored rows themselves (no image)
    const int img_kind = P.sel ? (int)IMG_NONE : h->img_kind;
    P.scan_dt = img_kind == IMG_F32S ? (int)F32S : h->dtype;
    ScanParams& sp = P.sp;
    plan_index_scan(h, P.sel != nullptr, nq, k, sp);
    h->last_plan[0] = sp.tr;
    h->last_plan[1] = sp.qt;
    h->last_plan[2] = sp.splits;
    P.nq_pad = round_up(nq, std::max<int64_t>(QPAD, sp.qt));  // whole scan tiles of (zero) queries
    const bool img = img_kind != IMG_NONE;
    if ((e = h->qw.f32.ensure((size_t)P.nq_pad * h->kdim * 4)) != hipSuccess) return e;
    if ((e = h->qw.op.ensure((size_t)P.nq_pad * h->row_bytes)) != hipSuccess) return e;
    if ((e = h->qw.eps.ensure((size_t)nq * 4)) != hipSuccess) return e;
    if ((e = h->qw.rho.ensure((size_t)nq * 4)) != hipSuccess) return e;
    if ((e = h->qw.shift.ensure((size_t)nq * 8)) != hipSuccess) return e;

    PrepParams& pp = P.pp;
    base_prep(h, h->qw, qdev, q_dtype, nq, P.nq_pad, P.scan_dt, pp);
    if (img) pp.img_bits = h->max_sq_bits + 1;
    pp.mu = img && h->centred ? (const float*)h->centre.p : nullptr;
    pp.qidx = nullptr;
    pp.nq_dev = nullptr;

    base_scan(h, img_kind, h->qw, nq, sp);
    sp.dbg = P.sel ? 0 : h->opt.scan_dbg;
    if ((e = h->gtau.ensure((size_t)P.nq_pad * 4)) != hipSuccess) return e;
    sp.gtau = (unsigned*)h->gtau.p;
    sp.conv = nullptr;
    // (only grids of more than one dispatch round: a single round's blocks
    // start together, and the word's read would only add a round trip to
    // the one-query call)
    if (!P.sel && h->opt.convoy != 0 && sp.grid > 256 && sp.splits <= CONV_MAX) {
        if (!h->conv.p) {
            if ((e = h->conv.ensure((size_t)CONV_WORDS * 4)) != hipSuccess) return e;
            if ((e = hipMemsetAsync(h->conv.p, 0, (size_t)CONV_WORDS * 4, h->stream())) != hipSuccess) return e;
        }
        sp.conv = (unsigned*)h->conv.p;
    }
    {
        const int ce = h->opt.convoy_every;
        sp.conv_every = ce >= 8 ? 8 : ce >= 4 ? 4 : ce >= 2 ? 2 : 1;
    }
    // k_scan_v4's published per-split lists (the union threshold, see
    // compact_wave): slow-path tiles 25.7 -> 16.5 %, config (d) -3 %
    if (sp.share && sp.splits > 1 && h->opt.pub != 0) {
        const size_t npub = (size_t)sp.n_qtiles * sp.qt * sp.splits * KP;
        if ((e = h->pub.ensure(npub * 4)) != hipSuccess) return e;
        sp.pub = (float*)h->pub.p;
        // union bound taken at rank max(6k/5, 12) (<= KP): tighter pruning;
        // the refine's certification bound is capped by the final threshold.
        // (k = 10: 12, was 20 -- config (b) -4.5 %, (d) -1 %, 0 fallbacks in
        // every certification stress case; profiles/r3/ab/prune_rank*)
        sp.prune_rank = h->opt.prune_rank > 0 ? h->opt.prune_rank : std::max(6 * k / 5, 12);
        sp.prune_rank = std::max(k, std::min(KP, sp.prune_rank));
    }
    P.ncand = (size_t)sp.n_qtiles * sp.splits * sp.qt * KP;
    if ((e = h->cand_d.ensure(P.ncand * 4)) != hipSuccess) return e;
    if ((e = h->cand_i.ensure(P.ncand * 4)) != hipSuccess) return e;
    sp.cand_d = (float*)h->cand_d.p;
    sp.cand_i = (int*)h->cand_i.p;
    sp.trace = nullptr;
    sp.dbgbuf = nullptr;
    sp.stamps = nullptr;
    sp.nq_dev = nullptr;

    if ((e = h->flag.ensure((size_t)(nq + 1) * 4)) != hipSuccess) return e;
    RefineParams& rp = P.rp;
    rp.cand_d = sp.cand_d;
    rp.cand_i = sp.cand_i;
    rp.splits = sp.splits;
    rp.qt = sp.qt;
    rp.nq = nq;
    rp.ntotal = h->ntotal;
    rp.k = k;
    rp.codes = h->codes;
    rp.row_bytes = h->row_bytes;
    rp.kdim = h->kdim;
    rp.qf32 = pp.qf32;
    rp.qeps = pp.qeps;
    rp.qrho = pp.qrho;
    rp.qshift = pp.qshift;
    rp.id_offset = h->id_offset;
    rp.labels = P.row_ids ? nullptr : h->label_ptr();
    rp.D = Dd;
    rp.I = Id;
    rp.n_flag = words ? words + 1 : (int*)h->flag.p;
    rp.flag_list = rp.n_flag + 1;
    rp.n_drop = words ? words : h->dev_drop;
    // small batches: one wave per query walks splits * KP candidates (256 splits
    // at nq = 1); issue 4 chunks of loads at a time (nq = 1: 0.84 -> ~0.3 ms)
    rp.prefetch = nq <= 256 ? 4 : 1;
    rp.k1 = big_k1(k);
    rp.force_fb = h->opt.force_fallback != 0;
    rp.gtau = sp.share ? sp.gtau : nullptr;
    rp.nq_dev = nullptr;
    rp.out_idx = nullptr;
    P.reduce = small_many(k, nq, sp.splits) && h->opt.reduce_cand == 2;
    rp.wg = small_many(k, nq, sp.splits) && h->opt.reduce_cand == 1 ? h->opt.refine_waves : 0;
    if (P.reduce) {
        const size_t nred = (size_t)sp.n_qtiles * ((sp.splits + 15) / 16) * sp.qt * KP;
        if ((e = h->cand2_d.ensure(nred * 4)) != hipSuccess) return e;
        if ((e = h->cand2_i.ensure(nred * 4)) != hipSuccess) return e;
    }
    const size_t nfb = (size_t)std::max<int64_t>(4096, nq) * k;
    if ((e = h->fbc_d.ensure(nfb * 4)) != hipSuccess) return e;
    if ((e = h->fbc_i.ensure(nfb * 4)) != hipSuccess) return e;
    return plan_rescan(h, P);
}

// the scan of a plan (pass 1's or the re-scan's parameters): the filtered
// kernel when the search has a selector
hipError_t run_scan(const FxIndex* h, const SearchPlan& P, const ScanParams& sp, hipStream_t s) {
    if (P.sel) return launch_scan_sel(h->dtype, h->metric, sp, P.sel->mask, P.sel->tiles, P.sel->cnt, s);
    return launch_scan(P.scan_dt, h->metric, sp, s);
}

// Enqueue the planned search on s up to its certification: query preparation
// (which also resets the shared thresholds, the published lists and the
// search's counters: one kernel instead of memsets), scan, refine +
// certification (small batches over many splits: one workgroup per query,
// or the separate candidate reduction when asked for).  No host sync: the
// same sequence is what a search graph captures.
hipError_t enqueue_main(FxIndex* h, SearchPlan& P, hipStream_t s, bool timed, hipEvent_t* ev) {
    hipError_t e;
    PrepParams pp1 = P.pp;
    pp1.gtau = P.sp.gtau;
    pp1.zero[0] = P.rp.n_drop;
    pp1.zero[1] = P.rp.n_flag;
    pp1.zero[2] = P.n_exact;
    pp1.pub = P.sp.pub;  // only live queries publish: nq rows of [splits][KP]
    pp1.npub = P.sp.pub ? P.nq * P.sp.splits * KP : 0;
    if ((e = launch_prep_queries(pp1, s)) != hipSuccess) return e;
    if (timed && (e = hipEventRecord(ev[0], s)) != hipSuccess) return e;
    if ((e = run_scan(h, P, P.sp, s)) != hipSuccess) return e;
    if (timed && (e = hipEventRecord(ev[1], s)) != hipSuccess) return e;
    RefineParams rp = P.rp;
    if (P.reduce) {
        int ng = 0;
        if ((e = launch_reduce_cand(P.sp.cand_d, P.sp.cand_i, P.sp.splits, P.nq, P.sp.qt, (float*)h->cand2_d.p,
                                    (int*)h->cand2_i.p, &ng, P.rp.ntotal, P.rp.n_drop, s)) != hipSuccess)
            return e;
        rp.cand_d = (const float*)h->cand2_d.p;
        rp.cand_i = (const int*)h->cand2_i.p;
        rp.splits = ng;
    }
    if ((e = launch_refine(h->dtype, h->metric, rp, s)) != hipSuccess) return e;
    if (timed && (e = hipEventRecord(ev[2], s)) != hipSuccess) return e;
    return hipSuccess;
}

// The chain for the queries the refine could not certify (rare: only when the
// candidate margin is inside the scan's rounding bound): a re-scan with a
// wide candidate set (plan_rescan), then the exact scan for what that still
// cannot certify.  Device-gated: every kernel reads the flagged count and
// exits at once when it is 0.  A device-resident search enqueues it always
// (no host round trip inside the search); a host-output search enqueues it
// only when its packed result says some query was flagged (finish_host_out).
hipError_t enqueue_fallback(FxIndex* h, SearchPlan& P, hipStream_t s) {
    hipError_t e;
#ifdef FX_ABLATION
    if ((P.sp.dbg & ~32) != 0) return hipSuccess;  // ablated scans: results invalid, no fallback chain
#endif
    if ((e = launch_rescan_chunks(P.rp.n_flag, (int)RESCAN_MAX, P.nchunks, P.chunk_cnt, s)) != hipSuccess) return e;
    for (int c = 0; c < P.nchunks; ++c) {  // chunk c: flagged queries [c RESCAN_MAX, ...)
        const int* list = P.rp.flag_list + (size_t)c * RESCAN_MAX;
        PrepParams pp = P.pp2;
        pp.qidx = list;
        pp.nq_dev = P.chunk_cnt + c;
        pp.zero[0] = pp.zero[1] = pp.zero[2] = nullptr;
        pp.pub = nullptr;
        pp.npub = 0;
        ScanParams sp = P.sp2;
        pp.gtau = sp.gtau;  // reset by the chunk's query preparation
        sp.nq_dev = P.chunk_cnt + c;
        RefineParams rp2 = P.rp2;
        rp2.nq_dev = P.chunk_cnt + c;
        rp2.out_idx = list;
        if ((e = launch_prep_queries(pp, s)) != hipSuccess) return e;
        if ((e = run_scan(h, P, sp, s)) != hipSuccess) return e;
        if ((e = launch_refine(h->dtype, h->metric, rp2, s)) != hipSuccess) return e;
    }
    return launch_exact_fallback(h->dtype, h->metric, h->codes, h->row_bytes, h->kdim, h->ntotal, P.rp.qf32,
                                 P.n_exact, P.k, h->id_offset, (float*)h->fbc_d.p, (int*)h->fbc_i.p, P.rp.D, P.rp.I,
                                 s, P.sel ? P.sel->mask : nullptr, P.rp.labels);
}

}  // namespace

// a host-output search whose refine dropped candidate ids outside [0, ntotal)
// (a corrupted scan list): the top-k may be missing rows, so it is an error
// (include/fx_index.h, fx_index_last_dropped_candidates)
int fx::integrity_error(const FxIndex* h) {
    return set_err(FX_E_INTEGRITY, "search: %lld candidate row ids outside [0, %lld) were dropped (corrupted scan list)",
                   (long long)h->last_dropped, (long long)h->ntotal);
}

namespace {

// Wait for a host-output search's results.  The one-query call is latency
// bound: polling the stream (host_spin) returns as soon as the D2H copy is
// done, where a blocking synchronise adds the runtime's wake-up latency.
hipError_t wait_results(const FxIndex* h, hipStream_t s) {
    if (!h->opt.host_spin) return hipStreamSynchronize(s);
    for (;;) {
        const hipError_t e = hipStreamQuery(s);
        if (e != hipErrorNotReady) return e;
    }
}

// A host-output search after its packed copy landed in `pin` (the stream is
// synchronised): when the refine flagged queries, run their fallback chain
// now and copy the results again (rare); then hand D / I to the caller.
int finish_host_out(FxIndex* h, SearchPlan& P, const HostOut& L, char* pin, float* D, int64_t* I) {
    hipStream_t s = h->stream();
    const int nflag = ((const int*)(pin + L.offW))[1];
    h->last_exact = 0;
    if (nflag > 0) {
        HIP_TRY(ensure_pinned_count(h));
        HIP_TRY(enqueue_fallback(h, P, s));
        HIP_TRY(hipMemcpyAsync(pin, P.rp.D, L.copy_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h->pin_nf + 1, P.n_exact, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        h->last_exact = h->pin_nf[1];
    }
    const int* w = (const int*)(pin + L.offW);
    memcpy(D, pin, (size_t)P.nq * P.k * 4);
    memcpy(I, pin + L.offI, (size_t)P.nq * P.k * 8);
    h->last_fallbacks = nflag;
    h->last_dropped = w[0];
    h->fb_pending = false;
    return h->last_dropped > 0 ? integrity_error(h) : FX_OK;
}

// host queries of a host-output search up to this size go through pinned
// staging (a memcpy and an async DMA instead of the runtime's pageable path:
// the one-query call is latency bound); the call waits for its results, so
// the staging buffer is free again when it returns
constexpr size_t QPIN_MAX = (size_t)4 << 20;

}  // namespace

int fx::do_search(FxIndex* h, int64_t nq, const void* q, int q_dtype, int q_mem, int k, float* D, int64_t* I,
                  int out_mem, const FxSelector* sel, bool row_ids) {
    hipStream_t s = h->stream();
    const int qes = dtype_size(q_dtype);
    // queries -> device
    const void* qdev = q;
    if (q_mem == FX_MEM_HOST) {
        const size_t qb = (size_t)nq * h->d * qes;
        HIP_TRY(h->qin.ensure(qb));
        if (out_mem == FX_MEM_HOST && qb <= QPIN_MAX && h->qpin.ensure(qb) == hipSuccess) {
            memcpy(h->qpin.p, q, qb);
            HIP_TRY(hipMemcpyAsync(h->qin.p, h->qpin.p, qb, hipMemcpyHostToDevice, s));
        } else {
            HIP_TRY(hipMemcpyAsync(h->qin.p, q, qb, hipMemcpyHostToDevice, s));
        }
        qdev = h->qin.p;
    }
    // host results: the packed output buffer (host_out_layout)
    const bool host_out = out_mem == FX_MEM_HOST;
    HostOut L;
    float* Dd = D;
    int64_t* Id = I;
    int* words = nullptr;
    if (host_out) {
        L = host_out_layout(nq, k);
        HIP_TRY(h->hout.ensure(L.bytes));
        HIP_TRY(h->hpin.ensure(L.copy_bytes));
        Dd = (float*)h->hout.p;
        Id = (int64_t*)((char*)h->hout.p + L.offI);
        words = (int*)((char*)h->hout.p + L.offW);
    }
    if (!sel) HIP_TRY(update_scan_image(h));  // (a filtered search reads no image)
    SearchPlan P;
    P.sel = sel;
    P.row_ids = row_ids;
    HIP_TRY(plan_search(h, nq, qdev, q_dtype, k, Dd, Id, words, P));
#ifdef FX_DIAG
    // diagnostics (Options): per-block placement/timing, phase stamps, the
    // scan's key matrix, raw candidate lists -> binary files
    const size_t grid = (size_t)P.sp.grid;
    if (!h->opt.stamps.empty()) {
        HIP_TRY(h->stamps.ensure(grid * 4 * 128));
        HIP_TRY(hipMemsetAsync(h->stamps.p, 0, grid * 4 * 128, s));
        P.sp.stamps = (unsigned long long*)h->stamps.p;
    }
    const size_t nkeys = (size_t)P.sp.n_qtiles * P.sp.qt * P.sp.n_ctiles * P.sp.tr;
    if ((P.sp.dbg & 32) && nkeys <= (size_t)1 << 26) {
        HIP_TRY(h->dbgbuf.ensure(nkeys * 4));
        HIP_TRY(hipMemsetAsync(h->dbgbuf.p, 0xff, nkeys * 4, s));
        P.sp.dbgbuf = (unsigned*)h->dbgbuf.p;
    }
    if (!h->opt.trace.empty()) {
        HIP_TRY(h->trace.ensure(grid * 32));
        HIP_TRY(hipMemsetAsync(h->trace.p, 0, grid * 32, s));
        P.sp.trace = (unsigned long long*)h->trace.p;
    }
#endif
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    if (h->profile)
        for (auto& x : ev) HIP_TRY(hipEventCreate(&x));
    HIP_TRY(enqueue_main(h, P, s, h->profile, ev));
    if (h->profile) {
        h->ev_scan.emplace_back(ev[0], ev[1]);
        h->ev_merge.emplace_back(ev[1], ev[2]);
    }
    if (!host_out) {
        // device results: the uncertified queries' chain is enqueued always and
        // decided on the device; the counts follow stream-ordered into pinned
        // memory, read only when asked for (read_counts)
        HIP_TRY(enqueue_fallback(h, P, s));
        HIP_TRY(ensure_pinned_count(h));
        HIP_TRY(hipMemcpyAsync(h->pin_nf, P.rp.n_flag, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h->pin_nf + 1, P.n_exact, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(h->pin_nf + 2, P.rp.n_drop, 4, hipMemcpyDeviceToHost, s));
        h->fb_pending = true;
    }
#ifdef FX_DIAG
    if (!h->opt.cand.empty()) {
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(dump_device<float>(h->opt.cand, P.sp.cand_d, P.ncand));
        HIP_TRY(dump_device<int>(h->opt.cand, P.sp.cand_i, P.ncand));
    }
    if (P.sp.dbgbuf) {  // the scan's key matrix [n_qtiles*128][n_ctiles*128]
        HIP_TRY(hipStreamSynchronize(s));
        const std::string path = h->opt.keys.empty() ? std::string("/tmp/fx_keys.bin") : h->opt.keys;
        if (FILE* f = fopen(path.c_str(), "wb")) fclose(f);  // truncate: one dump per search
        HIP_TRY(dump_device<float>(path, P.sp.dbgbuf, nkeys));
    }
    if (P.sp.stamps) {
        HIP_TRY(hipStreamSynchronize(s));
        if (FILE* f = fopen(h->opt.stamps.c_str(), "wb")) fclose(f);
        HIP_TRY(dump_device<unsigned long long>(h->opt.stamps, P.sp.stamps, grid * 4 * 16));
    }
    if (P.sp.trace) {
        HIP_TRY(hipStreamSynchronize(s));
        if (FILE* f = fopen(h->opt.trace.c_str(), "wb")) fclose(f);
        HIP_TRY(dump_device<unsigned long long>(h->opt.trace, P.sp.trace, grid * 4));
    }
#endif
    if (!host_out) return FX_OK;
    // host results: ONE packed D2H copy [D | I | n_drop | n_flag]
    HIP_TRY(hipMemcpyAsync(h->hpin.p, h->hout.p, L.copy_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(wait_results(h, s));
    return finish_host_out(h, P, L, (char*)h->hpin.p, D, I);
}

// k > FX_BIG_K: exact keys of every (query, row) pair and a radix sort per
// query (fx_hugek.hip).  Every result is exact, so no query is "uncertified".
constexpr size_t HK_KEEP_BYTES = (size_t)512 << 20;
int fx::do_search_hugek(FxIndex* h, int64_t nq, const void* q, int q_dtype, int q_mem, int k, float* D, int64_t* I,
                        int out_mem, bool row_ids) {
    hipStream_t s = h->stream();
    const void* qdev = nullptr;
    HIP_TRY(stage_in(h->stream(), h->qin, q, (size_t)nq * h->d * dtype_size(q_dtype), q_mem, &qdev));
    float* Dd = D;
    int64_t* Id = I;
    if (out_mem == FX_MEM_HOST) {
        HIP_TRY(h->dws.ensure((size_t)nq * k * 4));
        HIP_TRY(h->iws.ensure((size_t)nq * k * 8));
        Dd = (float*)h->dws.p;
        Id = (int64_t*)h->iws.p;
    }
    const int qb = hugek_batch(h->ntotal, nq);
    size_t ws = 0;
    HIP_TRY(hugek_workspace(h->ntotal, h->kdim, qb, &ws));
    HIP_TRY(h->hk.ws.ensure(ws));
    HugeKParams p{};
    p.codes = h->codes;
    p.row_bytes = h->row_bytes;
    p.kdim = h->kdim;
    p.d = h->d;
    p.st_dt = h->dtype;
    p.metric = h->metric;
    p.ntotal = h->ntotal;
    p.q = qdev;
    p.q_dt = q_dtype;
    p.nq = nq;
    p.k = k;
    p.id_offset = h->id_offset;
    p.labels = row_ids ? nullptr : h->label_ptr();
    p.D = Dd;
    p.I = Id;
    HIP_TRY(launch_hugek_search(p, h->hk.ws.p, h->hk.ws.bytes, qb, s));
    // the sort keys + rocPRIM temporaries stay cached for the next call up to
    // HK_KEEP_BYTES; a larger workspace (up to 2 GiB of keys) is released
    // after the call, which waits for the stream (hipFree would anyway)
    if (h->hk.ws.bytes > HK_KEEP_BYTES) {
        HIP_TRY(hipStreamSynchronize(s));
        h->hk.ws.release();
    }
    h->last_fallbacks = 0;
    h->last_exact = 0;
    h->last_dropped = 0;
    h->fb_pending = false;
    if (out_mem == FX_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(D, Dd, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(I, Id, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return FX_OK;
}

namespace {

// Shape + options + every device buffer a captured search touches: the graph
// is valid while all of them are unchanged
std::vector<uint64_t> graph_key(const FxIndex* h, int64_t nq, int q_dtype, int k) {
    const Options& o = h->opt;
    return {(uint64_t)nq, (uint64_t)q_dtype, (uint64_t)k, (uint64_t)h->ntotal, (uint64_t)h->id_offset,
            (uint64_t)h->img_kind, (uint64_t)h->centred, (uint64_t)h->img_rows,
            (uint64_t)o.force_fallback, (uint64_t)o.place, (uint64_t)o.sx, (uint64_t)o.reduce_cand,
            (uint64_t)o.pub, (uint64_t)o.prune_rank, (uint64_t)o.compact_at, (uint64_t)o.union_w,
            (uint64_t)o.union_defer, (uint64_t)(int64_t)o.union_inplace, (uint64_t)(int64_t)o.tight_at, (uint64_t)o.cold_bound,
            (uint64_t)o.reduce_cand, (uint64_t)o.scan_v5, (uint64_t)o.refine_waves, (uint64_t)o.convoy, (uint64_t)o.convoy_every,
            (uint64_t)(uintptr_t)h->codes.p, (uint64_t)(uintptr_t)h->norms.p, (uint64_t)(uintptr_t)h->split.p,
            (uint64_t)(uintptr_t)h->cnorms.p, (uint64_t)(uintptr_t)h->centre.p, (uint64_t)(uintptr_t)h->qw.shift.p,
            (uint64_t)(uintptr_t)h->qin.p, (uint64_t)(uintptr_t)h->qw.f32.p, (uint64_t)(uintptr_t)h->qw.op.p,
            (uint64_t)(uintptr_t)h->qw.eps.p, (uint64_t)(uintptr_t)h->qw.rho.p, (uint64_t)(uintptr_t)h->gtau.p,
            (uint64_t)(uintptr_t)h->pub.p, (uint64_t)(uintptr_t)h->cand_d.p, (uint64_t)(uintptr_t)h->cand_i.p,
            (uint64_t)(uintptr_t)h->cand2_d.p, (uint64_t)(uintptr_t)h->cand2_i.p,
            (uint64_t)(uintptr_t)h->hout.p, (uint64_t)(uintptr_t)h->conv.p,
            (uint64_t)(uintptr_t)h->flag.p, (uint64_t)(uintptr_t)h->fbc_d.p, (uint64_t)(uintptr_t)h->fbc_i.p,
            (uint64_t)(uintptr_t)h->rq.f32.p, (uint64_t)(uintptr_t)h->rq.op.p, (uint64_t)(uintptr_t)h->rq.eps.p,
            (uint64_t)(uintptr_t)h->rq.rho.p, (uint64_t)(uintptr_t)h->rq.shift.p, (uint64_t)(uintptr_t)h->rq.gtau.p,
            (uint64_t)(uintptr_t)h->rq.cand_d.p, (uint64_t)(uintptr_t)h->rq.cand_i.p,
            (uint64_t)(uintptr_t)h->rq.flag.p,
            // the label buffer the refine reads (null without labels): growth and a removal's swap replace it
            (uint64_t)(uintptr_t)h->label_ptr()};
}

}  // namespace

void fx::graph_release(FxIndex* h) {
    if (h->graph.exec) (void)hipGraphExecDestroy(h->graph.exec);
    h->graph.exec = nullptr;
    h->graph.key.clear();
}

namespace {

// Record the stream-ordered search of do_search (host queries, host results,
// no diagnostics) into h->graph.exec: the query's H2D copy, enqueue_main (prep,
// scan, refine: no fallback chain) and the packed result's one D2H copy.
// Runs right after a do_search of the same shape, so every workspace is
// sized and every kernel attribute set.
hipError_t graph_build(FxIndex* h, int64_t nq, int q_dtype, int k) {
    graph_release(h);
    hipStream_t s = h->stream();
    const size_t qb = (size_t)nq * h->d * dtype_size(q_dtype);
    const HostOut L = host_out_layout(nq, k);
    hipError_t e = hipSuccess;
    if ((e = h->graph.hq.ensure(qb)) != hipSuccess) return e;
    if ((e = h->graph.hout.ensure(L.copy_bytes)) != hipSuccess) return e;
    if ((e = h->hout.ensure(L.bytes)) != hipSuccess) return e;  // (sized by the do_search before)
    char* hb = (char*)h->hout.p;
    SearchPlan& P = h->graph.plan;
    P = SearchPlan{};
    if ((e = plan_search(h, nq, h->qin.p, q_dtype, k, (float*)hb, (int64_t*)(hb + L.offI), (int*)(hb + L.offW),
                         P)) != hipSuccess)
        return e;
    P.sp.dbg = 0;

    if ((e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal)) != hipSuccess) return e;
    g_graph_capture = true;
    hipError_t ce = hipMemcpyAsync(h->qin.p, h->graph.hq.p, qb, hipMemcpyHostToDevice, s);
    if (ce == hipSuccess) ce = enqueue_main(h, P, s, false, nullptr);
    if (ce == hipSuccess) ce = hipMemcpyAsync(h->graph.hout.p, hb, L.copy_bytes, hipMemcpyDeviceToHost, s);
    g_graph_capture = false;
    hipGraph_t graph = nullptr;
    e = hipStreamEndCapture(s, &graph);  // always end the capture: the stream must leave capture mode
    if (ce != hipSuccess) e = ce;
    if (e == hipSuccess) e = hipGraphInstantiate(&h->graph.exec, graph, nullptr, nullptr, 0);
    if (graph) (void)hipGraphDestroy(graph);
    if (e != hipSuccess) {
        h->graph.exec = nullptr;
        (void)hipGetLastError();
        return e;
    }
    h->graph.key = graph_key(h, nq, q_dtype, k);
    return hipSuccess;
}

// Small host batches under search_graph: replay the captured search; its
// fallback chain runs eagerly only when the packed result flags a query
// (finish_host_out).  On a shape / buffer / option change run do_search and
// re-capture.
int graph_search(FxIndex* h, int64_t nq, const void* q, int q_dtype, int k, float* D, int64_t* I) {
    HIP_TRY(update_scan_image(h));
    if (h->graph.exec && graph_key(h, nq, q_dtype, k) == h->graph.key) {
        hipStream_t s = h->stream();
        memcpy(h->graph.hq.p, q, (size_t)nq * h->d * dtype_size(q_dtype));
        HIP_TRY(hipGraphLaunch(h->graph.exec, s));
        HIP_TRY(wait_results(h, s));
        return finish_host_out(h, h->graph.plan, host_out_layout(nq, k), (char*)h->graph.hout.p, D, I);
    }
    const int rc = do_search(h, nq, q, q_dtype, FX_MEM_HOST, k, D, I, FX_MEM_HOST);
    if (rc == FX_OK && !h->graph.failed) {
        const hipError_t e = graph_build(h, nq, q_dtype, k);
        if (e != hipSuccess) {  // stay on do_search for this index
            h->graph.failed = true;
            if (h->opt.graph_verbose) fprintf(stderr, "fx: search graph capture failed: %s\n", hipGetErrorString(e));
        } else if (h->opt.graph_verbose) {
            fprintf(stderr, "fx: search graph captured (nq=%lld k=%d)\n", (long long)nq, k);
        }
    }
    return rc;
}

}  // namespace

// every slot missing (I = -1, D = FLT_MAX; IP: -FLT_MAX): the search of an
// empty index, or of an empty selection
int fx::fill_missing(FxIndex* h, int64_t nq, int k, float* D, int64_t* I, int out_mem) {
    const float dfill = h->metric == L2 ? FLT_MAX : -FLT_MAX;
    if (out_mem == FX_MEM_HOST) {
        std::fill(D, D + (size_t)nq * k, dfill);
        std::fill(I, I + (size_t)nq * k, (int64_t)-1);
    } else {  // stream-ordered fills: -1 is all ones in two's complement
        uint32_t bits;
        memcpy(&bits, &dfill, 4);
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)D, bits, (size_t)nq * k, h->stream()));
        HIP_TRY(hipMemsetAsync(I, 0xff, (size_t)nq * k * 8, h->stream()));
    }
    h->last_fallbacks = 0;
    h->last_exact = 0;
    h->last_dropped = 0;
    h->fb_pending = false;
    return FX_OK;
}

// the counts of the last search (after a device-resident one: synchronises the
// index stream, which is ordered after every stream the index used before)
int fx::read_counts(FxIndex* h) {
    if (h->fb_pending) {
        DeviceGuard g(h->device);
        HIP_TRY(hipStreamSynchronize(h->stream()));
        h->last_fallbacks = h->pin_nf[0];
        h->last_exact = h->pin_nf[1];
        h->last_dropped = h->pin_nf[2];
        h->fb_pending = false;
        if (h->last_dropped > 0) return integrity_error(h);
    }
    return FX_OK;
}

extern "C" {

int fx_index_search(FxIndex* h, int64_t nq, const void* q, int q_dtype, int q_mem, int k, float* D, int64_t* I,
                    int out_mem) {
    if (!h) return set_err(FX_E_ARG, "null index");
    if (nq < 0) return set_err(FX_E_ARG, "negative nq");
    if (k <= 0) return set_err(FX_E_ARG, "k must be positive (got %d)", k);
    static_assert(FX_MAX_K == FX_BIG_K, "ABI k limit of the scan path = the big-k refine's");
    if (!check_dtype(q_dtype)) return set_err(FX_E_ARG, "bad query dtype %d", q_dtype);
    if (nq == 0) return FX_OK;
    if (!q || !D || !I) return set_err(FX_E_ARG, "null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    if (h->ntotal > 0 && k > FX_MAX_K) return do_search_hugek(h, nq, q, q_dtype, q_mem, k, D, I, out_mem);
    if (h->ntotal == 0) return fill_missing(h, nq, k, D, I, out_mem);  // faiss: empty index -> every slot missing
    const Options& o = h->opt;
#ifdef FX_DIAG
    const bool diag = o.scan_dbg != 0 || !o.trace.empty() || !o.cand.empty() || !o.stamps.empty();
#else
    constexpr bool diag = false;
#endif
    if (o.search_graph == 1 && q_mem == FX_MEM_HOST && out_mem == FX_MEM_HOST && nq <= 64 && !h->profile && !diag &&
        h->user_stream == nullptr)
        return graph_search(h, nq, q, q_dtype, k, D, I);
    return do_search(h, nq, q, q_dtype, q_mem, k, D, I, out_mem);
}

int fx_index_last_dropped_candidates(FxIndex* h, int64_t* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    const int rc = read_counts(h);
    if (rc != FX_OK) return rc;
    *out = h->last_dropped;
    return FX_OK;
}

int fx_index_last_fallbacks(FxIndex* h, int64_t* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    const int rc = read_counts(h);
    if (rc != FX_OK) return rc;
    *out = h->last_fallbacks;
    return FX_OK;
}

int fx_index_last_scan_plan(FxIndex* h, int* tile_rows, int* query_tile, int* splits) {
    if (!h || !tile_rows || !query_tile || !splits) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *tile_rows = h->last_plan[0];
    *query_tile = h->last_plan[1];
    *splits = h->last_plan[2];
    return FX_OK;
}

int fx_index_last_exact_fallbacks(FxIndex* h, int64_t* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    const int rc = read_counts(h);
    if (rc != FX_OK) return rc;
    *out = h->last_exact;
    return FX_OK;
}

}  // extern "C"

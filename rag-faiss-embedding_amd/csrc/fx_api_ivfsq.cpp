// fx_api_ivfsq.cpp -- inverted file over 8-bit codes (fx_ivfsq.hip): fx_ivfsq_create / _train / _add /
// _search and the accessors.  The index owns its payload (codes, n_c, labels, the rows' lists) and its
// tables; the lists are the inverted file's (the quantizer's k = 1 search, the regroup of fx_ivf.hip),
// the rows the scalar quantizer's (fx_sq.hip's min / max training and encoder, fed with residuals).
// The handle and the row store are the shared ones (fx_host.h), the list state fx_ivf_lists.h's.
#include "fx_ivf_lists.h"

using namespace fx;

namespace {

constexpr int QT_8BIT = 0, QT_8BIT_UNIFORM = 2;
// rows per chunk of train / add: the quantizer's chunk, and at most 256 MiB of fp32 residuals
int64_t ivfsq_chunk(const FxIvfSq* v, int64_t n) {
    const int64_t kc = v->quant->opt.kmeans_chunk > 0 ? v->quant->opt.kmeans_chunk : (int)KMEANS_CHUNK_DEFAULT;
    const int64_t rc = std::max<int64_t>(1, (256ll << 20) / ((int64_t)v->d * 4));
    return std::max<int64_t>(1, std::min(n, std::min(kc, rc)));
}

int ivfsq_need_trained(const FxIvfSq* v, const char* who) {
    if (const int rc = ivf_quant_trained(*v, who); rc != FX_OK) return rc;
    if (!v->trained) return set_err(FX_E_ARG, "%s: the index is not trained (no scalar-quantizer tables)", who);
    return FX_OK;
}

// cent <- the quantizer's rows widened to fp32 (what its reconstruct returns)
int ivfsq_fetch_centroids(FxIvfSq* v) {
    if (!v->by_residual) return FX_OK;
    hipStream_t s = v->stream();
    HIP_TRY(v->cent.ensure((size_t)v->nlist * v->d * 4));
    BorrowQuant bq(v->quant, s);
    HIP_TRY(bq.begin());
    HIP_TRY(launch_to_f32(v->quant->codes, v->quant->dtype, v->quant->row_bytes, v->nlist, v->d, v->cent, s));
    return FX_OK;
}

// lists of x [nr][d] (on the device) -> out[nr] as launch_ivf_record stores them
int ivfsq_assign(FxIvfSq* v, int64_t nr, const void* xd, int x_dtype, int* out) {
    hipStream_t s = v->stream();
    HIP_TRY(v->assign.ensure((size_t)nr * 12));
    int64_t* a = (int64_t*)v->assign.p;
    float* dd = (float*)((char*)v->assign.p + (size_t)nr * 8);
    {
        BorrowQuant bq(v->quant, s);
        HIP_TRY(bq.begin());
        const int rc = do_search(v->quant, nr, xd, x_dtype, FX_MEM_DEVICE, 1, dd, a, FX_MEM_DEVICE);
        if (rc != FX_OK) return rc;
    }
    HIP_TRY(launch_ivf_record(a, nr, v->nlist, out, v->bad + 1, s));
    return FX_OK;
}

int regroup(FxIvfSq* v) {
    const IvfRows rows{v->ntotal, v->cap_rows, v->stride, v->codes, v->nc, v->labels, v->row_list};
    return ivf_regroup("ivfsq", *v, rows, true, v->bad + 1, v->stream());
}

}  // namespace

extern "C" {

int fx_ivfsq_create(FxIndex* quantizer, int d, int64_t nlist, int qtype, int metric, int by_residual, FxIvfSq** out) {
    if (!out) return set_err(FX_E_ARG, "null out");
    *out = nullptr;
    if (d <= 0) return set_err(FX_E_ARG, "dimension must be positive (got %d)", d);
    if (nlist < 1) return set_err(FX_E_ARG, "ivfsq: nlist must be positive (got %lld)", (long long)nlist);
    if (nlist >= (int64_t)INT32_MAX) return set_err(FX_E_UNSUPPORTED, "ivfsq: more than 2^31-2 lists");
    if (qtype != QT_8BIT && qtype != QT_8BIT_UNIFORM)
        return set_err(FX_E_ARG, "ivfsq: qtype %d is not offered (0 QT_8bit, 2 QT_8bit_uniform)", qtype);
    if (metric != FX_METRIC_L2 && metric != FX_METRIC_INNER_PRODUCT) return set_err(FX_E_ARG, "bad metric %d", metric);
    if (!quantizer) return set_err(FX_E_ARG, "ivfsq: null quantizer");
    if (quantizer->d != d)
        return set_err(FX_E_ARG, "ivfsq: the quantizer has d = %d, the index d = %d", quantizer->d, d);
    if (quantizer->has_ids) return set_err(FX_E_ARG, "ivfsq: the quantizer carries labels (add_with_ids)");
    if (quantizer->id_offset != 0)
        return set_err(FX_E_ARG, "ivfsq: the quantizer has id offset %lld", (long long)quantizer->id_offset);
    DeviceGuard g(quantizer->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", quantizer->device);
    FxIvfSq* v = new FxIvfSq();
    v->quant = quantizer;
    v->d = d;
    v->qtype = qtype;
    v->metric = metric;
    v->by_residual = by_residual != 0;
    v->device = quantizer->device;
    v->nlist = nlist;
    v->stride = (int)round_up(d, ROW_ALIGN);
    v->lists = true;
    v->h_off.assign((size_t)nlist + 1, 0);
    hipError_t e = v->init();
    if (e == hipSuccess) e = v->tables.ensure((size_t)2 * d * 4);
    if (e == hipSuccess) e = v->mm.ensure((size_t)2 * d * 4);
    if (e == hipSuccess) e = v->words.ensure(SQ_WORDS * 4);
    if (e == hipSuccess) e = hipMemset(v->words, 0, SQ_WORDS * 4);
    if (e == hipSuccess) e = v->list_off.ensure((size_t)(nlist + 1) * 4);
    if (e == hipSuccess) e = hipMemset(v->list_off, 0, (size_t)(nlist + 1) * 4);
    if (e == hipSuccess) e = v->max_rows.ensure(16);
    if (e == hipSuccess) e = v->bad.ensure(16);
    if (e == hipSuccess) e = hipMemset(v->bad, 0, 16);
    if (e != hipSuccess) {
        fx_ivfsq_free(v);
        return set_err(FX_E_HIP, "ivfsq init: %s", hipGetErrorString(e));
    }
    *out = v;
    return FX_OK;
}

void fx_ivfsq_free(FxIvfSq* v) { handle_free(v); }

int fx_ivfsq_train(FxIvfSq* v, int64_t n, const void* x, int x_dtype, int x_mem, int more) {
    // (the handle last: the other checks are then reachable without a device)
    if (const int rc = check_rows(n, x_dtype, x_mem); rc != FX_OK) return rc;
    if (!v) return set_err(FX_E_ARG, "null ivfsq index");
    std::lock_guard<std::mutex> lk(v->mu);
    if (v->ntotal > 0)
        return set_err(FX_E_ARG, "ivfsq train: the index holds %lld rows (reset it first)", (long long)v->ntotal);
    if (const int rc = ivf_quant_trained(*v, "ivfsq train"); rc != FX_OK) return rc;
    if (n == 0 && !v->train_open) return FX_OK;
    if (n > 0 && !x) return set_err(FX_E_ARG, "null x");
    DeviceGuard g(v->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", v->device);
    hipStream_t s = v->stream();
    if (!v->train_open) {
        if (const int rc = ivfsq_fetch_centroids(v); rc != FX_OK) return rc;
        HIP_TRY(launch_sq_minmax_reset(v->mm, v->d, v->bad, s));
        HIP_TRY(hipMemsetAsync(v->bad + 1, 0, 8, s));
        v->train_open = true;
        v->trained = false;
    }
    const int rc = staged_rows(
        s, v->in, n, x, (size_t)v->d * dtype_size(x_dtype), x_mem, ivfsq_chunk(v, n),
        [&](const void* xd, int64_t, int64_t nr) {
            if (!v->by_residual) {
                HIP_TRY(launch_sq_minmax(xd, x_dtype, nr, v->d, v->mm, v->bad, s));
                return (int)FX_OK;
            }
            HIP_TRY(v->tlist.ensure((size_t)nr * 4));
            HIP_TRY(v->resid.ensure((size_t)nr * v->d * 4));
            if (const int rc = ivfsq_assign(v, nr, xd, x_dtype, (int*)v->tlist.p); rc != FX_OK) return rc;
            HIP_TRY(launch_ivfsq_residual(xd, x_dtype, nr, v->d, (const int*)v->tlist.p, v->nlist, v->cent,
                                          (float*)v->resid.p, s));
            HIP_TRY(launch_sq_minmax(v->resid.p, F32, nr, v->d, v->mm, v->bad, s));
            return (int)FX_OK;
        });
    if (rc != FX_OK || more) return rc;
    // the one synchronisation of a training: its non-finite and unassigned counts
    unsigned long long bad[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(bad, v->bad, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(v->bad, 0, 16, s));
    HIP_TRY(hipStreamSynchronize(s));
    v->train_open = false;
    if (bad[0] > 0) return set_err(FX_E_ARG, "ivfsq train: %llu non-finite values in the training data", bad[0]);
    if (bad[1] > 0) return ivf_bad_error("ivfsq", (int64_t)bad[1], v->nlist);
    HIP_TRY(launch_sq_finish(v->mm, v->d, v->qtype == QT_8BIT_UNIFORM, v->tables, s));
    HIP_TRY(launch_ivfsq_consts(v->tables, v->d, v->by_residual ? (const float*)v->cent : nullptr, v->nlist, v->words, s));
    v->trained = true;
    return FX_OK;
}

int fx_ivfsq_is_trained(const FxIvfSq* v, int* out) {
    if (!v || !out) return set_err(FX_E_ARG, "null argument");
    *out = v->trained ? 1 : 0;
    return FX_OK;
}

int fx_ivfsq_get_trained(FxIvfSq* v, float* out) {
    if (!v || !out) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(v->mu);
    if (!v->trained) return set_err(FX_E_ARG, "ivfsq get_trained: the index is not trained");
    DeviceGuard g(v->device);
    return finish_out(v->stream(), out, v->tables, (size_t)2 * v->d * 4, FX_MEM_HOST);
}

int fx_ivfsq_set_trained(FxIvfSq* v, const float* trained) {
    if (!v || !trained) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(v->mu);
    if (v->ntotal > 0)
        return set_err(FX_E_ARG, "ivfsq set_trained: the index holds %lld rows (reset it first)", (long long)v->ntotal);
    if (const int rc = ivf_quant_trained(*v, "ivfsq set_trained"); rc != FX_OK) return rc;
    if (const int rc = sq_check_tables("ivfsq", v->d, trained); rc != FX_OK) return rc;
    DeviceGuard g(v->device);
    hipStream_t s = v->stream();
    if (const int rc = ivfsq_fetch_centroids(v); rc != FX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(v->tables, trained, (size_t)2 * v->d * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(launch_ivfsq_consts(v->tables, v->d, v->by_residual ? (const float*)v->cent : nullptr, v->nlist, v->words, s));
    v->train_open = false;
    v->trained = true;
    return FX_OK;
}

int fx_ivfsq_add(FxIvfSq* v, int64_t n, const void* x, int x_dtype, int x_mem, const int64_t* ids, int ids_mem) {
    if (const int rc = check_rows(n, x_dtype, x_mem); rc != FX_OK) return rc;
    if (ids && !valid_mem(ids_mem)) return set_err(FX_E_ARG, "bad ids_mem %d", ids_mem);
    if (!v) return set_err(FX_E_ARG, "null ivfsq index");
    if (n == 0) return FX_OK;
    if (!x) return set_err(FX_E_ARG, "null x");
    std::lock_guard<std::mutex> lk(v->mu);
    if (const int rc = ivfsq_need_trained(v, "ivfsq add"); rc != FX_OK) return rc;
    if (const int rc = ivf_add_mode(*v, v->ntotal, ids); rc != FX_OK) return rc;
    if (v->ntotal + n + 2 * TILE_R >= (int64_t)INT32_MAX)
        return set_err(FX_E_UNSUPPORTED, "ivfsq: more than 2^31-1 rows");
    DeviceGuard g(v->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", v->device);
    hipStream_t s = v->stream();
    HIP_TRY(v->grow(v->ntotal + n, s));
    const int rb = v->stride;
    const int arc = staged_rows(
        s, v->in, n, x, (size_t)v->d * dtype_size(x_dtype), x_mem, ivfsq_chunk(v, n),
        [&](const void* xd, int64_t r0, int64_t nr) {
            const int64_t row0 = v->ntotal + r0;
            if (const int rc = ivfsq_assign(v, nr, xd, x_dtype, v->row_list + row0); rc != FX_OK) return rc;
            const void* src = xd;
            int src_dt = x_dtype;
            if (v->by_residual) {
                HIP_TRY(v->resid.ensure((size_t)nr * v->d * 4));
                HIP_TRY(launch_ivfsq_residual(xd, x_dtype, nr, v->d, v->row_list + row0, v->nlist, v->cent,
                                              (float*)v->resid.p, s));
                src = v->resid.p;
                src_dt = F32;
            }
            HIP_TRY(launch_sq_encode(src, src_dt, nr, v->d, v->tables, rb, v->codes + (size_t)row0 * rb, v->nc + row0,
                                     v->words, s));
            return (int)FX_OK;
        });
    if (arc != FX_OK) return arc;
    if (ids) {
        HIP_TRY(hipMemcpyAsync(v->labels + v->ntotal, ids, (size_t)n * 8,
                               ids_mem == FX_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
        if (ids_mem == FX_MEM_HOST) HIP_TRY(hipStreamSynchronize(s));  // (the caller's array may go)
    } else {
        HIP_TRY(launch_ivf_iota(v->labels + v->ntotal, n, v->ntotal, s));
    }
    if (v->ntotal == 0) v->sequential = ids == nullptr;
    v->ntotal += n;
    v->dirty = true;
    if (x_mem == FX_MEM_HOST) {  // a host call waits for its work: its skipped rows are known now
        int64_t bad = 0;
        if (const int rc = ivf_read_bad(v->bad + 1, s, &bad); rc != FX_OK) return rc;
        if (bad > 0) return ivf_bad_error("ivfsq", bad, v->nlist);
    }
    return FX_OK;
}

int fx_ivfsq_search(FxIvfSq* v, int64_t nq, const void* q, int q_dtype, int q_mem, int k, int nprobe, float* D,
                    int64_t* I, int out_mem) {
    if (const int rc = ivf_search_args("ivfsq", nq, k, nprobe, q_dtype, q_mem, out_mem); rc != FX_OK) return rc;
    if (!v) return set_err(FX_E_ARG, "null ivfsq index");
    std::lock_guard<std::mutex> lk(v->mu);
    if (const int rc = ivfsq_need_trained(v, "ivfsq search"); rc != FX_OK) return rc;
    if (nq == 0) return FX_OK;
    if (!q || !D || !I) return set_err(FX_E_ARG, "null buffer");
    int np = 0;
    if (const int rc = ivf_probes("ivfsq", *v, nq, nprobe, &np); rc != FX_OK) return rc;
    DeviceGuard g(v->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", v->device);
    if (const int rc = regroup(v); rc != FX_OK) return rc;
    // (an earlier device search's counts, if nobody asked for them, give way to this search's)
    v->clear_counts();
    hipStream_t s = v->stream();
    if (v->ntotal == 0) return fill_missing(s, v->metric, nq, k, D, I, out_mem);

    const int rb = v->stride;
    const IvfSqPlan P = plan_ivfsq(nq, np, v->nlist, v->max_list_rows, v->ntotal, k, rb);
    const int qes = dtype_size(q_dtype);
    const void* qdev = nullptr;
    HIP_TRY(stage_in(s, v->qin, q, (size_t)nq * v->d * qes, q_mem, &qdev));
    void *Dd = D, *Id = I;
    HIP_TRY(out_buf(v->outD, D, (size_t)nq * k * 4, out_mem, &Dd));
    HIP_TRY(out_buf(v->outI, I, (size_t)nq * k * 8, out_mem, &Id));
    HIP_TRY(hipMemsetAsync(v->cnt, 0, 16, s));
    const int C = P.chunks, slots = P.slots;
    const bool fused = P.path == IVF_PATH_FUSED;
    const int64_t qb_max = std::min(P.q_batch, nq);
    const int64_t pad_max = round_up(qb_max * np, TILE_Q);
    HIP_TRY(ivf_search_workspace(*v, P, nq, np, k));
    HIP_TRY(v->qf32.ensure((size_t)qb_max * rb * 4));
    if (fused) {
        HIP_TRY(v->planes.ensure((size_t)SQ_P * pad_max * rb));
        HIP_TRY(v->sigma.ensure((size_t)pad_max * 4));
        HIP_TRY(v->peps.ensure((size_t)pad_max * 4));
        HIP_TRY(v->pshift.ensure((size_t)pad_max * 4));
    }
    int* n_flag = (int*)v->flag.p;
    const float* cent = v->by_residual ? (const float*)v->cent : nullptr;

    for (int64_t q0 = 0; q0 < nq; q0 += qb_max) {
        const int64_t qb = std::min(qb_max, nq - q0);
        const void* qp = (const char*)qdev + (size_t)q0 * v->d * qes;
        hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        HIP_TRY(v->begin_pass(ev, 5, s));
        // 1. coarse: the quantizer's exact top-np search names the probed lists
        if (const int rc = ivf_coarse(*v, s, qb, qp, q_dtype, np); rc != FX_OK) return rc;
        HIP_TRY(v->mark(ev[1], s));
        IvfSqExact ex{};
        ex.ex.codes = v->codes;
        ex.ex.row_bytes = rb;
        ex.ex.kdim = rb;
        ex.ex.list_off = v->list_off;
        ex.ex.nlist = v->nlist;
        ex.ex.coarse = (const int64_t*)v->coarse_i.p;
        ex.ex.np = np;
        ex.ex.C = C;
        ex.ex.qf32 = (const float*)v->qf32.p;
        ex.ex.n_flag = n_flag;
        ex.ex.k = k;
        ex.ex.cd = (float*)v->cand_d.p;
        ex.ex.ci = (int*)v->cand_i.p;
        ex.ex.labels = v->labels;
        ex.ex.D = (float*)Dd + q0 * k;
        ex.ex.I = (int64_t*)Id + q0 * k;
        ex.d = v->d;
        ex.trained = v->tables;
        ex.cent = cent;
        if (!fused) {
            // the exact path for the whole pass: every query "flagged"
            HIP_TRY(launch_f32_queries(qp, q_dtype, qb, v->d, rb, (float*)v->qf32.p, s));
            HIP_TRY(launch_ivf_count_bad(ex.ex.coarse, qb * np, v->nlist, v->cnt + 2, s));
            HIP_TRY(launch_ivf_flag_all(n_flag, qb, s));
            HIP_TRY(v->mark(ev[2], s));
            HIP_TRY(launch_ivfsq_exact(v->metric, ex, s));
            HIP_TRY(v->mark(ev[3], s));  // (the exact scan is this path's "list scan"; it has no refine)
            HIP_TRY(v->mark(ev[4], s));
            continue;
        }
        // 2. the pass's (query, list) pairs grouped by list, and their operands
        HIP_TRY(ivf_pairs(*v, v->cnt + 2, qb, np, s));
        const int64_t pairs_pad = round_up(qb * np, TILE_Q);
        IvfSqPrep pp{};
        pp.q = qp;
        pp.q_dt = q_dtype;
        pp.metric = v->metric;
        pp.d = v->d;
        pp.row_bytes = rb;
        pp.nq = qb;
        pp.np = np;
        pp.pairs_pad = pairs_pad;
        pp.coarse = ex.ex.coarse;
        pp.nlist = v->nlist;
        pp.cent = cent;
        pp.trained = v->tables;
        pp.words = v->words;
        pp.qf32 = (float*)v->qf32.p;
        pp.planes = (char*)v->planes.p;
        pp.sigma = (float*)v->sigma.p;
        pp.peps = (float*)v->peps.p;
        pp.pshift = (float*)v->pshift.p;
        pp.zero[0] = n_flag;
        pp.zero[1] = nullptr;
        HIP_TRY(launch_ivfsq_prep(pp, s));
        // 3. the list scan; slots no block writes hold id -1
        HIP_TRY(hipMemsetAsync(v->cand_i.p, 0xff, (size_t)qb * slots * KP * 4, s));
        IvfSqScan sc{};
        sc.codes = v->codes;
        sc.nc = v->nc;
        sc.row_bytes = rb;
        sc.list_off = v->list_off;
        sc.nlist = v->nlist;
        sc.planes = pp.planes;
        sc.sigma = pp.sigma;
        sc.pshift = pp.pshift;
        sc.pairs_pad = pairs_pad;
        sc.np = np;
        sc.C = C;
        sc.sorted = (uint64_t*)v->psorted.p;
        sc.seg = (int*)v->seg.p;
        sc.gbase = (int*)v->gbase.p;
        sc.cand_d = (float*)v->cand_d.p;
        sc.cand_i = (int*)v->cand_i.p;
        sc.grid = (qb * np / TILE_Q + std::min<int64_t>(v->nlist, qb * np)) * C;
        HIP_TRY(v->mark(ev[2], s));
        HIP_TRY(launch_ivfsq_scan(v->metric, sc, s));
        HIP_TRY(v->mark(ev[3], s));
#ifdef FX_DIAG
        // FX_IVFSQ_CAND (read when the index was created): the pass's scan lists, probed lists, list
        // offsets, pair operands and row constants appended to the file, before the refine reads the
        // lists and the exact scan writes over them:
        //   cand_d, cand_i [qb][slots][KP] | coarse [qb][np] i64 | list_off [nlist + 1] |
        //   sigma, pshift, peps [pairs_pad] | planes [3][pairs_pad][row_bytes] | n_c [ntotal]
        if (!v->opt.ivfsq_cand.empty()) {
            const std::string& path = v->opt.ivfsq_cand;
            HIP_TRY(hipStreamSynchronize(s));
            HIP_TRY(dump_device<float>(path, sc.cand_d, (size_t)qb * slots * KP));
            HIP_TRY(dump_device<int>(path, sc.cand_i, (size_t)qb * slots * KP));
            HIP_TRY(dump_device<int64_t>(path, ex.ex.coarse, (size_t)qb * np));
            HIP_TRY(dump_device<int>(path, v->list_off, (size_t)v->nlist + 1));
            HIP_TRY(dump_device<float>(path, pp.sigma, (size_t)pairs_pad));
            HIP_TRY(dump_device<float>(path, pp.pshift, (size_t)pairs_pad));
            HIP_TRY(dump_device<float>(path, pp.peps, (size_t)pairs_pad));
            HIP_TRY(dump_device<char>(path, pp.planes, (size_t)SQ_P * pairs_pad * rb));
            HIP_TRY(dump_device<float>(path, v->nc, (size_t)v->ntotal));
        }
#endif
        // 4. refine + certification over the query's slots
        IvfSqRefine rp{};
        rp.cand_d = sc.cand_d;
        rp.cand_i = sc.cand_i;
        rp.slots = slots;
        rp.np = np;
        rp.nq = qb;
        rp.ntotal = v->ntotal;
        rp.k = k;
        rp.d = v->d;
        rp.row_bytes = rb;
        rp.codes = v->codes;
        rp.row_list = v->row_list;
        rp.nlist = v->nlist;
        rp.cent = cent;
        rp.trained = v->tables;
        rp.words = v->words;
        rp.qf32 = pp.qf32;
        rp.peps = pp.peps;
        rp.labels = v->labels;
        rp.D = ex.ex.D;
        rp.I = ex.ex.I;
        rp.n_flag = n_flag;
        rp.n_drop = v->cnt;
        rp.force_fb = v->opt.force_fallback != 0;
        HIP_TRY(launch_ivfsq_refine(v->metric, rp, s));
        // 5. the flagged queries' exact lists (device-gated; the candidate buffers are free again)
        HIP_TRY(launch_ivfsq_exact(v->metric, ex, s));
        HIP_TRY(launch_ivf_accum(v->cnt + 1, n_flag, s));
        HIP_TRY(v->mark(ev[4], s));
    }
    return ivf_search_finish("ivfsq", *v, *v, v->device, s, nq, k, D, Dd, I, Id, out_mem, v->ntotal);
}

int fx_ivfsq_reset(FxIvfSq* v) {
    if (!v) return set_err(FX_E_ARG, "null ivfsq index");
    std::lock_guard<std::mutex> lk(v->mu);
    DeviceGuard g(v->device);
    hipStream_t s = v->stream();
    HIP_TRY(hipStreamSynchronize(s));
    // the maxima restart; the decode bound and the tables belong to the training and stay
    HIP_TRY(hipMemsetAsync(v->words, 0, 8, s));
    HIP_TRY(v->zero(s));
    HIP_TRY(hipMemsetAsync(v->list_off, 0, (size_t)(v->nlist + 1) * 4, s));
    HIP_TRY(hipMemsetAsync(v->bad + 1, 0, 8, s));
    v->h_off.assign((size_t)v->nlist + 1, 0);
    v->ntotal = 0;
    v->max_list_rows = 0;
    v->dirty = false;
    v->sequential = false;
    v->clear_counts();
    return FX_OK;
}

int fx_ivfsq_ntotal(const FxIvfSq* v, int64_t* out) {
    if (!v || !out) return set_err(FX_E_ARG, "null argument");
    *out = v->ntotal;
    return FX_OK;
}

int fx_ivfsq_list_sizes(FxIvfSq* v, int64_t* out) { return ivf_list_sizes(v, regroup, out); }

int fx_ivfsq_list_ids(FxIvfSq* v, int64_t list, int64_t* out, int64_t cap, int64_t* n) {
    if (!v) return set_err(FX_E_ARG, "null argument");
    return ivf_list_ids(v, "ivfsq", regroup, v->labels, list, out, cap, n);
}

int fx_ivfsq_list_codes(FxIvfSq* v, int64_t list, uint8_t* out, int64_t cap, int64_t* n) {
    if (!v || !n) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(v->mu);
    if (list < 0 || list >= v->nlist)
        return set_err(FX_E_ARG, "ivfsq list_codes: list %lld outside [0, %lld)", (long long)list, (long long)v->nlist);
    DeviceGuard g(v->device);
    if (const int rc = regroup(v); rc != FX_OK) return rc;
    const int64_t r0 = v->h_off[list], cnt = (int64_t)v->h_off[list + 1] - r0;
    *n = cnt;
    if (cnt == 0 || cap <= 0) return FX_OK;
    if (!out) return set_err(FX_E_ARG, "null buffer");
    const int64_t take = std::min(cnt, cap);
    hipStream_t s = v->stream();
    HIP_TRY(v->io.ensure((size_t)take * v->d));
    HIP_TRY(launch_ivfsq_codes_u8(v->codes, v->stride, r0, take, v->d, (uint8_t*)v->io.p, s));
    return finish_out(s, out, v->io.p, (size_t)take * v->d, FX_MEM_HOST);
}

int fx_ivfsq_set_stream(FxIvfSq* v, void* stream) { return handle_set_stream(v, "ivfsq", stream); }

int fx_ivfsq_last_counts(FxIvfSq* v, int64_t* fallbacks, int64_t* exact_fallbacks, int64_t* dropped) {
    return handle_last_counts(v, v ? v->quant : nullptr, fallbacks, exact_fallbacks, dropped);
}

int fx_ivfsq_last_plan(FxIvfSq* v, int* path, int* chunks, int* slots, int64_t* q_batch, int64_t* grid) {
    return ivf_last_plan(v, path, chunks, slots, q_batch, grid);
}

int fx_ivfsq_profile(FxIvfSq* v, int enable) { return handle_profile(v, "ivfsq", enable); }

int fx_ivfsq_profile_read(FxIvfSq* v, double* coarse_ms, double* pairs_ms, double* scan_ms, double* refine_ms,
                          int64_t* passes) {
    double* const ms[] = {coarse_ms, pairs_ms, scan_ms, refine_ms};
    return handle_profile_read(v, ms, passes);
}

}  // extern "C"

// fx_api_ivfpq.cpp -- inverted file over product-quantized codes (fx_ivfpq.hip): fx_ivfpq_create /
// _set_centroids / _residuals / _add / _search and the accessors.  The index owns its payload (codes,
// n_y, labels, the rows' lists) and its codebook; the lists are the inverted file's (the quantizer's k
// = 1 search, the regroup of fx_ivf.hip), the rows the product quantizer's (fx_pq.hip's encoder and row
// constant, fed with residuals).  Training is the caller's: fx_ivfpq_residuals hands out what the
// codebook is trained on, fx_ivfpq_set_centroids installs it.  The handle and the row store are the
// shared ones (fx_host.h), the list state fx_ivf_lists.h's, the codebook's host side fx_api_pq.cpp's.
#include "fx_ivf_lists.h"

using namespace fx;

namespace {

// rows per chunk of residuals / add: the quantizer's chunk, and at most 256 MiB of fp32 residuals
int64_t ivfpq_chunk(const FxIvfPq* v, int64_t n) {
    const int64_t kc = v->quant->opt.kmeans_chunk > 0 ? v->quant->opt.kmeans_chunk : (int)KMEANS_CHUNK_DEFAULT;
    const int64_t rc = std::max<int64_t>(1, (256ll << 20) / ((int64_t)v->d * 4));
    return std::max<int64_t>(1, std::min(n, std::min(kc, rc)));
}

int ivfpq_need_trained(const FxIvfPq* v, const char* who) {
    if (const int rc = ivf_quant_trained(*v, who); rc != FX_OK) return rc;
    if (!v->trained) return set_err(FX_E_ARG, "%s: the index is not trained (no codebook)", who);
    return FX_OK;
}

// cent <- the quantizer's rows widened to fp32 (what its reconstruct returns)
int ivfpq_fetch_centroids(FxIvfPq* v) {
    if (!v->by_residual) return FX_OK;
    hipStream_t s = v->stream();
    HIP_TRY(v->cent.ensure((size_t)v->nlist * v->d * 4));
    BorrowQuant bq(v->quant, s);
    HIP_TRY(bq.begin());
    HIP_TRY(launch_to_f32(v->quant->codes, v->quant->dtype, v->quant->row_bytes, v->nlist, v->d, v->cent, s));
    return FX_OK;
}

// lists of x [nr][d] (on the device) -> out[nr] as launch_ivf_record stores them
int ivfpq_assign(FxIvfPq* v, int64_t nr, const void* xd, int x_dtype, int* out) {
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

int regroup(FxIvfPq* v) {
    const IvfRows rows{v->ntotal, v->cap_rows, v->stride, v->codes, v->nc, v->labels, v->row_list};
    return ivf_regroup("ivfpq", *v, rows, true, v->bad + 1, v->stream());
}

}  // namespace

extern "C" {

int fx_ivfpq_create(FxIndex* quantizer, int d, int64_t nlist, int M, int nbits, int metric, int by_residual,
                    FxIvfPq** out) {
    if (!out) return set_err(FX_E_ARG, "null out");
    *out = nullptr;
    if (d <= 0) return set_err(FX_E_ARG, "dimension must be positive (got %d)", d);
    if (nlist < 1) return set_err(FX_E_ARG, "ivfpq: nlist must be positive (got %lld)", (long long)nlist);
    if (nlist >= (int64_t)INT32_MAX) return set_err(FX_E_UNSUPPORTED, "ivfpq: more than 2^31-2 lists");
    if (M <= 0 || M > 65535 || d % M != 0)
        return set_err(FX_E_ARG, "ivfpq: d = %d is not a multiple of M = %d (1 <= M <= 65535)", d, M);
    if (nbits != 8) return set_err(FX_E_UNSUPPORTED, "ivfpq: nbits = %d is not offered (8)", nbits);
    if (metric != FX_METRIC_L2 && metric != FX_METRIC_INNER_PRODUCT) return set_err(FX_E_ARG, "bad metric %d", metric);
    if (!quantizer) return set_err(FX_E_ARG, "ivfpq: null quantizer");
    if (quantizer->d != d)
        return set_err(FX_E_ARG, "ivfpq: the quantizer has d = %d, the index d = %d", quantizer->d, d);
    if (quantizer->has_ids) return set_err(FX_E_ARG, "ivfpq: the quantizer carries labels (add_with_ids)");
    if (quantizer->id_offset != 0)
        return set_err(FX_E_ARG, "ivfpq: the quantizer has id offset %lld", (long long)quantizer->id_offset);
    DeviceGuard g(quantizer->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", quantizer->device);
    FxIvfPq* v = new FxIvfPq();
    v->quant = quantizer;
    v->d = d;
    v->M = M;
    v->dsub = d / M;
    v->kp = pq_kpad(d);
    v->metric = metric;
    v->by_residual = by_residual != 0;
    v->device = quantizer->device;
    v->nlist = nlist;
    v->stride = pq_stride(M);
    v->lists = true;
    v->h_off.assign((size_t)nlist + 1, 0);
    hipError_t e = v->init();
    if (e == hipSuccess) e = v->cb.ensure((size_t)M * PQ_KSUB * v->dsub * 4);
    if (e == hipSuccess && v->dsub % 8 == 0) e = v->img.ensure((size_t)2 * pq_plane_bytes(M, v->dsub));
    if (e == hipSuccess) e = v->list_off.ensure((size_t)(nlist + 1) * 4);
    if (e == hipSuccess) e = hipMemset(v->list_off, 0, (size_t)(nlist + 1) * 4);
    if (e == hipSuccess) e = v->max_rows.ensure(16);
    if (e == hipSuccess) e = v->bad.ensure(16);
    if (e == hipSuccess) e = hipMemset(v->bad, 0, 16);
    if (e != hipSuccess) {
        fx_ivfpq_free(v);
        return set_err(FX_E_HIP, "ivfpq init: %s", hipGetErrorString(e));
    }
    *out = v;
    return FX_OK;
}

void fx_ivfpq_free(FxIvfPq* v) { handle_free(v); }

int fx_ivfpq_is_trained(const FxIvfPq* v, int* out) {
    if (!v || !out) return set_err(FX_E_ARG, "null argument");
    *out = v->trained ? 1 : 0;
    return FX_OK;
}

int fx_ivfpq_get_centroids(FxIvfPq* v, float* out) {
    if (!v || !out) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(v->mu);
    if (const int rc = need_trained(v->trained, "ivfpq", "get_centroids"); rc != FX_OK) return rc;
    memcpy(out, v->h_cb.data(), v->h_cb.size() * 4);
    return FX_OK;
}

int fx_ivfpq_set_centroids(FxIvfPq* v, const float* centroids) {
    if (!v || !centroids) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(v->mu);
    if (v->ntotal > 0)
        return set_err(FX_E_ARG, "ivfpq set_centroids: the index holds %lld rows (reset it first)", (long long)v->ntotal);
    if (const int rc = ivf_quant_trained(*v, "ivfpq set_centroids"); rc != FX_OK) return rc;
    const int M = v->M, dsub = v->dsub, d = v->d;
    const size_t nval = (size_t)M * PQ_KSUB * dsub;
    PqCodebook cbk;
    if (const int rc = pq_codebook("ivfpq", M, dsub, centroids, cbk); rc != FX_OK) return rc;
    DeviceGuard g(v->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", v->device);
    hipStream_t s = v->stream();
    HIP_TRY(hipStreamSynchronize(s));  // (an earlier search may still read the image)
    if (const int rc = ivfpq_fetch_centroids(v); rc != FX_OK) return rc;
    // rho_dec of y = fl32(c_l + decode): per dimension u (max_l |c_lj| + max_j |centroid value|), root of
    // the sum of squares, so it holds for any list and any code
    double rho2 = 0.0;
    if (v->by_residual) {
        std::vector<float> hc((size_t)v->nlist * d);
        HIP_TRY(hipMemcpyAsync(hc.data(), v->cent, hc.size() * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const double u = 5.9604644775390625e-8;  // 2^-24
        for (int j = 0; j < d; ++j) {
            double cmax = 0.0, ymax = 0.0;
            for (int64_t l = 0; l < v->nlist; ++l) cmax = std::max(cmax, std::fabs((double)hc[(size_t)l * d + j]));
            const int m = j / dsub, e = j - m * dsub;
            for (int c = 0; c < PQ_KSUB; ++c)
                ymax = std::max(ymax, std::fabs((double)centroids[((size_t)m * PQ_KSUB + c) * dsub + e]));
            if (!std::isfinite(cmax)) return set_err(FX_E_ARG, "ivfpq set_centroids: the quantizer holds a non-finite centroid");
            const double dj = u * (cmax + ymax) * 1.001;
            rho2 += dj * dj;
        }
    }
    HIP_TRY(hipMemcpyAsync(v->cb, centroids, nval * 4, hipMemcpyHostToDevice, s));
    if (!cbk.img.empty()) HIP_TRY(hipMemcpyAsync(v->img, cbk.img.data(), cbk.img.size() * 2, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    v->h_cb.assign(centroids, centroids + nval);
    v->Y = cbk.Y;
    v->Ry = cbk.Ry;
    v->Yl = cbk.Yl;
    v->rho_dec = std::sqrt(rho2) * 1.000001;
    v->trained = true;
    return FX_OK;
}

int fx_ivfpq_residuals(FxIvfPq* v, int64_t n, const void* x, int x_dtype, int x_mem, float* out, int out_mem) {
    if (const int rc = check_rows(n, x_dtype, x_mem); rc != FX_OK) return rc;
    if (!valid_mem(out_mem)) return set_err(FX_E_ARG, "bad out_mem %d", out_mem);
    if (!v) return set_err(FX_E_ARG, "null ivfpq index");
    if (n == 0) return FX_OK;
    if (!x || !out) return set_err(FX_E_ARG, "null buffer");
    std::lock_guard<std::mutex> lk(v->mu);
    if (const int rc = ivf_quant_trained(*v, "ivfpq residuals"); rc != FX_OK) return rc;
    DeviceGuard g(v->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", v->device);
    hipStream_t s = v->stream();
    // (before the codebook is set the centroids are read afresh; afterwards they are the training's)
    if (!v->trained)
        if (const int rc = ivfpq_fetch_centroids(v); rc != FX_OK) return rc;
    const int rc = staged_rows(
        s, v->in, n, x, (size_t)v->d * dtype_size(x_dtype), x_mem, ivfpq_chunk(v, n),
        [&](const void* xd, int64_t r0, int64_t nr) {
            const size_t bytes = (size_t)nr * v->d * 4;
            float* o = out + (size_t)r0 * v->d;
            void* od = o;
            HIP_TRY(out_buf(v->io, o, bytes, out_mem, &od));
            if (v->by_residual) {
                HIP_TRY(v->tlist.ensure((size_t)nr * 4));
                if (const int rc = ivfpq_assign(v, nr, xd, x_dtype, (int*)v->tlist.p); rc != FX_OK) return rc;
                HIP_TRY(launch_ivfsq_residual(xd, x_dtype, nr, v->d, (const int*)v->tlist.p, v->nlist, v->cent, (float*)od, s));
            } else {
                HIP_TRY(launch_f32_queries(xd, x_dtype, nr, v->d, v->d, (float*)od, s));
            }
            return finish_out(s, o, od, bytes, out_mem);
        });
    if (rc != FX_OK) return rc;
    if (x_mem == FX_MEM_HOST || out_mem == FX_MEM_HOST) {  // a host call waits: its unassigned rows are known now
        int64_t bad = 0;
        if (const int rc = ivf_read_bad(v->bad + 1, s, &bad); rc != FX_OK) return rc;
        if (bad > 0) return ivf_bad_error("ivfpq", bad, v->nlist);
    }
    return FX_OK;
}

int fx_ivfpq_add(FxIvfPq* v, int64_t n, const void* x, int x_dtype, int x_mem, const int64_t* ids, int ids_mem) {
    if (const int rc = check_rows(n, x_dtype, x_mem); rc != FX_OK) return rc;
    if (ids && !valid_mem(ids_mem)) return set_err(FX_E_ARG, "bad ids_mem %d", ids_mem);
    if (!v) return set_err(FX_E_ARG, "null ivfpq index");
    if (n == 0) return FX_OK;
    if (!x) return set_err(FX_E_ARG, "null x");
    std::lock_guard<std::mutex> lk(v->mu);
    if (const int rc = ivfpq_need_trained(v, "ivfpq add"); rc != FX_OK) return rc;
    if (const int rc = ivf_add_mode(*v, v->ntotal, ids); rc != FX_OK) return rc;
    if (v->ntotal + n + 2 * TILE_R >= (int64_t)INT32_MAX)
        return set_err(FX_E_UNSUPPORTED, "ivfpq: more than 2^31-1 rows");
    DeviceGuard g(v->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", v->device);
    hipStream_t s = v->stream();
    HIP_TRY(v->grow(v->ntotal + n, s));
    const int st = v->stride;
    const int arc = staged_rows(
        s, v->in, n, x, (size_t)v->d * dtype_size(x_dtype), x_mem, ivfpq_chunk(v, n),
        [&](const void* xd, int64_t r0, int64_t nr) {
            const int64_t row0 = v->ntotal + r0;
            if (const int rc = ivfpq_assign(v, nr, xd, x_dtype, v->row_list + row0); rc != FX_OK) return rc;
            const void* src = xd;
            int src_dt = x_dtype;
            if (v->by_residual) {
                HIP_TRY(v->resid.ensure((size_t)nr * v->d * 4));
                HIP_TRY(launch_ivfsq_residual(xd, x_dtype, nr, v->d, v->row_list + row0, v->nlist, v->cent,
                                              (float*)v->resid.p, s));
                src = v->resid.p;
                src_dt = F32;
            }
            uint8_t* c0 = v->u8() + (size_t)row0 * st;
            HIP_TRY(launch_pq_encode(src, src_dt, nr, v->d, v->M, v->dsub, v->cb, c0, st, s));
            HIP_TRY(launch_pq_ny(c0, st, nr, v->M, v->dsub, v->cb, v->nc + row0, s));
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
        if (bad > 0) return ivf_bad_error("ivfpq", bad, v->nlist);
    }
    return FX_OK;
}

int fx_ivfpq_search(FxIvfPq* v, int64_t nq, const void* q, int q_dtype, int q_mem, int k, int nprobe, float* D,
                    int64_t* I, int out_mem) {
    if (const int rc = ivf_search_args("ivfpq", nq, k, nprobe, q_dtype, q_mem, out_mem); rc != FX_OK) return rc;
    if (!v) return set_err(FX_E_ARG, "null ivfpq index");
    std::lock_guard<std::mutex> lk(v->mu);
    if (const int rc = ivfpq_need_trained(v, "ivfpq search"); rc != FX_OK) return rc;
    if (nq == 0) return FX_OK;
    if (!q || !D || !I) return set_err(FX_E_ARG, "null buffer");
    int np = 0;
    if (const int rc = ivf_probes("ivfpq", *v, nq, nprobe, &np); rc != FX_OK) return rc;
    DeviceGuard g(v->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", v->device);
    if (const int rc = regroup(v); rc != FX_OK) return rc;
    // (an earlier device search's counts, if nobody asked for them, give way to this search's)
    v->clear_counts();
    hipStream_t s = v->stream();
    if (v->ntotal == 0) return fill_missing(s, v->metric, nq, k, D, I, out_mem);

    const int st = v->stride, kp = v->kp;
    // L2 with by_residual: the operand holds the list's centroid, one per pair; else one per query
    const bool per_pair = v->by_residual && v->metric == L2;
    const IvfPqPlan P = plan_ivfpq(nq, np, v->nlist, v->max_list_rows, v->ntotal, k, v->d, v->dsub, per_pair ? 1 : 0);
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
    const int64_t op_max = per_pair ? pad_max : round_up(qb_max, TILE_Q);
    HIP_TRY(ivf_search_workspace(*v, P, nq, np, k));
    HIP_TRY(v->qf32.ensure((size_t)qb_max * kp * 4));
    if (fused) {
        HIP_TRY(v->planes.ensure((size_t)2 * op_max * kp * 2));
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
        IvfPqExact ex{};
        ex.ex.codes = v->codes;
        ex.ex.row_bytes = st;
        ex.ex.kdim = kp;
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
        ex.dsub = v->dsub;
        ex.cb = v->cb;
        ex.cent = cent;
        if (!fused) {
            // the exact path for the whole pass: every query "flagged"
            HIP_TRY(launch_f32_queries(qp, q_dtype, qb, v->d, kp, (float*)v->qf32.p, s));
            HIP_TRY(launch_ivf_count_bad(ex.ex.coarse, qb * np, v->nlist, v->cnt + 2, s));
            HIP_TRY(launch_ivf_flag_all(n_flag, qb, s));
            HIP_TRY(v->mark(ev[2], s));
            HIP_TRY(launch_ivfpq_exact(v->metric, ex, s));
            HIP_TRY(v->mark(ev[3], s));  // (the exact scan is this path's "list scan"; it has no refine)
            HIP_TRY(v->mark(ev[4], s));
            continue;
        }
        // 2. the pass's (query, list) pairs grouped by list, and their operands
        HIP_TRY(ivf_pairs(*v, v->cnt + 2, qb, np, s));
        const int64_t pairs_pad = round_up(qb * np, TILE_Q);
        const int64_t op_rows = per_pair ? pairs_pad : round_up(qb, TILE_Q);
        IvfPqPrep pp{};
        pp.q = qp;
        pp.q_dt = q_dtype;
        pp.metric = v->metric;
        pp.d = v->d;
        pp.kp = kp;
        pp.nq = qb;
        pp.np = np;
        pp.per_pair = per_pair ? 1 : 0;
        pp.op_rows = op_rows;
        pp.coarse = ex.ex.coarse;
        pp.nlist = v->nlist;
        pp.cent = cent;
        pp.Y = v->Y;
        pp.Ry = v->Ry;
        pp.Yl = v->Yl;
        pp.rho_dec = v->by_residual ? v->rho_dec : 0.0;
        pp.qf32 = (float*)v->qf32.p;
        pp.planes = (uint16_t*)v->planes.p;
        pp.peps = (float*)v->peps.p;
        pp.pshift = (float*)v->pshift.p;
        pp.zero[0] = n_flag;
        pp.zero[1] = nullptr;
        HIP_TRY(launch_ivfpq_prep(pp, s));
        // 3. the list scan; slots no block writes hold id -1
        HIP_TRY(hipMemsetAsync(v->cand_i.p, 0xff, (size_t)qb * slots * KP * 4, s));
        IvfPqScan sc{};
        sc.codes = v->u8();
        sc.ny = v->nc;
        sc.stride = st;
        sc.M = v->M;
        sc.dsub = v->dsub;
        sc.d = v->d;
        sc.kp = kp;
        sc.img = v->img;
        sc.plane_bytes = pq_plane_bytes(v->M, v->dsub);
        sc.list_off = v->list_off;
        sc.nlist = v->nlist;
        sc.planes = pp.planes;
        sc.op_rows = op_rows;
        sc.bdiv = per_pair ? 1 : np;
        sc.pshift = pp.pshift;
        sc.np = np;
        sc.C = C;
        sc.sorted = (uint64_t*)v->psorted.p;
        sc.seg = (int*)v->seg.p;
        sc.gbase = (int*)v->gbase.p;
        sc.cand_d = (float*)v->cand_d.p;
        sc.cand_i = (int*)v->cand_i.p;
        sc.grid = (qb * np / TILE_Q + std::min<int64_t>(v->nlist, qb * np)) * C;
        HIP_TRY(v->mark(ev[2], s));
        HIP_TRY(launch_ivfpq_scan(v->metric, sc, s));
        HIP_TRY(v->mark(ev[3], s));
#ifdef FX_DIAG
        // FX_IVFPQ_CAND (read when the index was created): the pass's scan lists, probed lists, list
        // offsets, pair operands and rows appended to the file, before the refine reads the lists and the
        // exact scan writes over them:
        //   cand_d, cand_i [qb][slots][KP] | coarse [qb][np] i64 | list_off [nlist + 1] |
        //   pshift, peps [pairs_pad] | planes [2][op_rows][kp] bf16 | codes [ntotal][stride] u8 | n_y [ntotal]
        if (!v->opt.ivfpq_cand.empty()) {
            const std::string& path = v->opt.ivfpq_cand;
            HIP_TRY(hipStreamSynchronize(s));
            HIP_TRY(dump_device<float>(path, sc.cand_d, (size_t)qb * slots * KP));
            HIP_TRY(dump_device<int>(path, sc.cand_i, (size_t)qb * slots * KP));
            HIP_TRY(dump_device<int64_t>(path, ex.ex.coarse, (size_t)qb * np));
            HIP_TRY(dump_device<int>(path, v->list_off, (size_t)v->nlist + 1));
            HIP_TRY(dump_device<float>(path, pp.pshift, (size_t)pairs_pad));
            HIP_TRY(dump_device<float>(path, pp.peps, (size_t)pairs_pad));
            HIP_TRY(dump_device<uint16_t>(path, pp.planes, (size_t)2 * op_rows * kp));
            HIP_TRY(dump_device<uint8_t>(path, v->codes, (size_t)v->ntotal * st));
            HIP_TRY(dump_device<float>(path, v->nc, (size_t)v->ntotal));
        }
#endif
        // 4. refine + certification over the query's slots
        IvfPqRefine rp{};
        rp.cand_d = sc.cand_d;
        rp.cand_i = sc.cand_i;
        rp.slots = slots;
        rp.np = np;
        rp.nq = qb;
        rp.ntotal = v->ntotal;
        rp.k = k;
        rp.d = v->d;
        rp.kp = kp;
        rp.dsub = v->dsub;
        rp.stride = st;
        rp.codes = v->u8();
        rp.cb = v->cb;
        rp.row_list = v->row_list;
        rp.nlist = v->nlist;
        rp.cent = cent;
        rp.rho_dec = pp.rho_dec;
        rp.qf32 = pp.qf32;
        rp.peps = pp.peps;
        rp.labels = v->labels;
        rp.D = ex.ex.D;
        rp.I = ex.ex.I;
        rp.n_flag = n_flag;
        rp.n_drop = v->cnt;
        rp.force_fb = v->opt.force_fallback != 0;
        HIP_TRY(launch_ivfpq_refine(v->metric, rp, s));
        // 5. the flagged queries' exact lists (device-gated; the candidate buffers are free again)
        HIP_TRY(launch_ivfpq_exact(v->metric, ex, s));
        HIP_TRY(launch_ivf_accum(v->cnt + 1, n_flag, s));
        HIP_TRY(v->mark(ev[4], s));
    }
    return ivf_search_finish("ivfpq", *v, *v, v->device, s, nq, k, D, Dd, I, Id, out_mem, v->ntotal);
}

int fx_ivfpq_reset(FxIvfPq* v) {
    if (!v) return set_err(FX_E_ARG, "null ivfpq index");
    std::lock_guard<std::mutex> lk(v->mu);
    DeviceGuard g(v->device);
    hipStream_t s = v->stream();
    HIP_TRY(hipStreamSynchronize(s));
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

int fx_ivfpq_ntotal(const FxIvfPq* v, int64_t* out) {
    if (!v || !out) return set_err(FX_E_ARG, "null argument");
    *out = v->ntotal;
    return FX_OK;
}

int fx_ivfpq_list_sizes(FxIvfPq* v, int64_t* out) { return ivf_list_sizes(v, regroup, out); }

int fx_ivfpq_list_ids(FxIvfPq* v, int64_t list, int64_t* out, int64_t cap, int64_t* n) {
    if (!v) return set_err(FX_E_ARG, "null argument");
    return ivf_list_ids(v, "ivfpq", regroup, v->labels, list, out, cap, n);
}

int fx_ivfpq_list_codes(FxIvfPq* v, int64_t list, uint8_t* out, int64_t cap, int64_t* n) {
    if (!v || !n) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(v->mu);
    if (list < 0 || list >= v->nlist)
        return set_err(FX_E_ARG, "ivfpq list_codes: list %lld outside [0, %lld)", (long long)list, (long long)v->nlist);
    DeviceGuard g(v->device);
    if (const int rc = regroup(v); rc != FX_OK) return rc;
    const int64_t r0 = v->h_off[list], cnt = (int64_t)v->h_off[list + 1] - r0;
    *n = cnt;
    if (cnt == 0 || cap <= 0) return FX_OK;
    if (!out) return set_err(FX_E_ARG, "null buffer");
    const int64_t take = std::min(cnt, cap);
    hipStream_t s = v->stream();
    // the rows' first M bytes, densely: faiss's [.][M]
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)v->M, v->codes + (size_t)r0 * v->stride, (size_t)v->stride, (size_t)v->M,
                             (size_t)take, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FX_OK;
}

int fx_ivfpq_set_stream(FxIvfPq* v, void* stream) { return handle_set_stream(v, "ivfpq", stream); }

int fx_ivfpq_last_counts(FxIvfPq* v, int64_t* fallbacks, int64_t* exact_fallbacks, int64_t* dropped) {
    return handle_last_counts(v, v ? v->quant : nullptr, fallbacks, exact_fallbacks, dropped);
}

int fx_ivfpq_last_plan(FxIvfPq* v, int* path, int* chunks, int* slots, int64_t* q_batch, int64_t* grid) {
    return ivf_last_plan(v, path, chunks, slots, q_batch, grid);
}

int fx_ivfpq_profile(FxIvfPq* v, int enable) { return handle_profile(v, "ivfpq", enable); }

int fx_ivfpq_profile_read(FxIvfPq* v, double* coarse_ms, double* pairs_ms, double* scan_ms, double* refine_ms,
                          int64_t* passes) {
    double* const ms[] = {coarse_ms, pairs_ms, scan_ms, refine_ms};
    return handle_profile_read(v, ms, passes);
}

}  // extern "C"

// fx_api_ivf.cpp -- inverted file (fx_ivf.hip): fx_ivf_create / _add / _search and the accessors.
//
// The payload (FxIvf::pay) is a labelled flat index this file drives directly:
// rows and labels are appended to its tail by fx_index_add_with_ids, each new
// row's list is recorded from the quantizer's k = 1 search, and the next search
// regroups the rows into list order (a stable sort of list << 32 | row keys and a
// gather into second buffers that are then swapped in).  The regroup needs a
// second copy of the payload while it runs (released again once the buffers
// are swapped) and is O(ntotal) per add-then-search cycle; merging only the
// appended tail is future work.
#include "fx_ivf_lists.h"

using namespace fx;

namespace fx {

int ivf_quant_trained(const IvfLists& L, const char* who) {
    if (L.quant->ntotal != L.nlist)
        return set_err(FX_E_ARG, "%s: the index is not trained (the quantizer holds %lld of %lld centroids)", who,
                       (long long)L.quant->ntotal, (long long)L.nlist);
    return FX_OK;
}

int ivf_bad_error(const char* kind, int64_t bad, int64_t nlist) {
    return set_err(FX_E_INTEGRITY, "%s: %lld rows were assigned outside [0, %lld) and belong to no list", kind,
                   (long long)bad, (long long)nlist);
}

int ivf_read_bad(unsigned long long* bad, hipStream_t s, int64_t* out) {
    unsigned long long h_bad = 0;
    HIP_TRY(hipMemcpyAsync(&h_bad, bad, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(bad, 0, 8, s));
    HIP_TRY(hipStreamSynchronize(s));
    *out = (int64_t)h_bad;
    return FX_OK;
}

int ivf_add_mode(const IvfLists& L, int64_t ntotal, const int64_t* ids) {
    if (ntotal > 0 && L.sequential && ids)
        return set_err(FX_E_ARG, "add_with_ids not implemented for an index that holds rows without labels");
    if (ntotal > 0 && !L.sequential && !ids)
        return set_err(FX_E_ARG, "add does not make sense on an index with labels: use add_with_ids");
    return FX_OK;
}

int ivf_regroup(const char* kind, IvfLists& L, const IvfRows& R, bool zero_incoming, unsigned long long* bad,
                hipStream_t s) {
    if (!L.dirty) return FX_OK;
    L.h_off.assign((size_t)L.nlist + 1, 0);
    if (R.n == 0) {
        HIP_TRY(hipMemsetAsync(L.list_off, 0, (size_t)(L.nlist + 1) * 4, s));
        L.max_list_rows = 0;
        L.dirty = false;
        return FX_OK;
    }
    // the second copy of the payload: released again when this call returns
    DevBuf codes, norms, labels, row_list;
    HIP_TRY(codes.ensure((size_t)R.cap_rows * R.row_bytes));
    HIP_TRY(norms.ensure((size_t)R.cap_rows * 4));
    HIP_TRY(labels.ensure(std::max<size_t>((size_t)R.cap_rows * 8, R.labels.bytes)));
    HIP_TRY(row_list.ensure(std::max<size_t>((size_t)R.cap_rows * 4, R.row_list.bytes)));
    if (zero_incoming) {
        HIP_TRY(hipMemsetAsync(codes.p, 0, codes.bytes, s));
        HIP_TRY(hipMemsetAsync(norms.p, 0, norms.bytes, s));
    }
    size_t ws = 0;
    HIP_TRY(ivf_regroup_bytes(R.n, L.nlist, &ws));
    HIP_TRY(L.rws.ensure(ws));
    IvfRegroup r{};
    r.n = R.n;
    r.nlist = L.nlist;
    r.row_bytes = R.row_bytes;
    r.codes = (const char*)R.codes.p;
    r.norms = (const float*)R.norms.p;
    r.labels = (const int64_t*)R.labels.p;
    r.row_list = (const int*)R.row_list.p;
    r.dst_codes = (char*)codes.p;
    r.dst_norms = (float*)norms.p;
    r.dst_labels = (int64_t*)labels.p;
    r.dst_row_list = (int*)row_list.p;
    r.list_off = L.list_off;
    r.max_rows = L.max_rows;
    HIP_TRY(launch_ivf_regroup(r, L.rws.p, L.rws.bytes, s));
    // the one synchronisation: the longest list (the planner's input), with the lists' offsets
    int max_rows = 0;
    HIP_TRY(hipMemcpyAsync(&max_rows, L.max_rows, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(L.h_off.data(), L.list_off, (size_t)(L.nlist + 1) * 4, hipMemcpyDeviceToHost, s));
    int64_t nbad = 0;
    if (const int rc = ivf_read_bad(bad, s, &nbad); rc != FX_OK) return rc;
    // (the stream is idle: nothing reads the buffers that go out)
    R.codes.swap(codes);
    R.norms.swap(norms);
    R.labels.swap(labels);
    R.row_list.swap(row_list);
    L.max_list_rows = max_rows;
    L.dirty = false;
    if (nbad > 0) return ivf_bad_error(kind, nbad, L.nlist);
    return FX_OK;
}

int ivf_search_args(const char* kind, int64_t nq, int k, int nprobe, int q_dtype, int q_mem, int out_mem) {
    if (nq < 0) return set_err(FX_E_ARG, "negative nq");
    if (k < 1) return set_err(FX_E_ARG, "k must be positive (got %d)", k);
    if (nprobe < 1) return set_err(FX_E_ARG, "nprobe must be positive (got %d)", nprobe);
    if (!check_dtype(q_dtype)) return set_err(FX_E_ARG, "bad query dtype %d", q_dtype);
    if (!valid_mem(q_mem) || !valid_mem(out_mem)) return set_err(FX_E_ARG, "bad q_mem / out_mem");
    if (k > FX_MAX_K) return set_err(FX_E_UNSUPPORTED, "%s search: k = %d above FX_MAX_K = %d", kind, k, FX_MAX_K);
    return FX_OK;
}

int ivf_probes(const char* kind, const IvfLists& L, int64_t nq, int nprobe, int* np) {
    *np = (int)std::min<int64_t>(nprobe, L.nlist);
    if (nq * *np >= (int64_t)INT32_MAX)
        return set_err(FX_E_UNSUPPORTED, "%s search: nq * nprobe = %lld pairs (limit 2^31-1)", kind, (long long)(nq * *np));
    if (*np > FX_MAX_K)
        return set_err(FX_E_UNSUPPORTED, "%s search: nprobe = %d above %d (the coarse search's k)", kind, *np, FX_MAX_K);
    return FX_OK;
}

hipError_t ivf_search_workspace(IvfLists& L, const IvfPlan& P, int64_t nq, int np, int k) {
    L.last_plan[0] = P.path;
    L.last_plan[1] = P.chunks;
    L.last_plan[2] = P.slots;
    L.last_qbatch = P.q_batch;
    L.last_grid = P.grid;
    const bool fused = P.path == IVF_PATH_FUSED;
    const int64_t qb_max = std::min(P.q_batch, nq);
    const size_t ncand = (size_t)qb_max * P.slots * (fused ? KP : k), nl = (size_t)(L.nlist + 1) * 4;
    hipError_t e = L.coarse_d.ensure((size_t)qb_max * np * 4);
    if (e == hipSuccess) e = L.coarse_i.ensure((size_t)qb_max * np * 8);
    if (e == hipSuccess) e = L.flag.ensure((size_t)(qb_max + 1) * 4);
    if (e == hipSuccess) e = L.cand_d.ensure(ncand * 4);
    if (e == hipSuccess) e = L.cand_i.ensure(ncand * 4);
    if (e != hipSuccess || !fused) return e;
    e = L.pkeys.ensure((size_t)qb_max * np * 8);
    if (e == hipSuccess) e = L.psorted.ensure((size_t)qb_max * np * 8);
    if (e == hipSuccess) e = L.seg.ensure(nl);
    if (e == hipSuccess) e = L.ngrp.ensure(nl);
    if (e == hipSuccess) e = L.gbase.ensure(nl);
    // hipCUB's temporaries for every pass size that occurs: full passes and a shorter last one
    size_t tb = 0, tb_last = 0;
    if (e == hipSuccess) e = ivf_pairs_temp_bytes(qb_max * np, L.nlist, &tb);
    if (e == hipSuccess && nq % qb_max != 0) e = ivf_pairs_temp_bytes((nq % qb_max) * np, L.nlist, &tb_last);
    if (e == hipSuccess) e = L.ptemp.ensure(std::max<size_t>(std::max(tb, tb_last), 16));
    return e;
}

int ivf_coarse(IvfLists& L, hipStream_t s, int64_t qb, const void* q, int q_dtype, int np) {
    BorrowQuant bq(L.quant, s);
    HIP_TRY(bq.begin());
    return do_search(L.quant, qb, q, q_dtype, FX_MEM_DEVICE, np, (float*)L.coarse_d.p, (int64_t*)L.coarse_i.p,
                     FX_MEM_DEVICE);
}

hipError_t ivf_pairs(IvfLists& L, int* bad_cnt, int64_t qb, int np, hipStream_t s) {
    IvfPairs pr{};
    pr.coarse = (const int64_t*)L.coarse_i.p;
    pr.npairs = qb * np;
    pr.nlist = L.nlist;
    pr.list_off = L.list_off;
    pr.keys = (uint64_t*)L.pkeys.p;
    pr.sorted = (uint64_t*)L.psorted.p;
    pr.seg = (int*)L.seg.p;
    pr.ngrp = (int*)L.ngrp.p;
    pr.gbase = (int*)L.gbase.p;
    pr.bad = bad_cnt;
    return launch_ivf_pairs(pr, L.ptemp.p, L.ptemp.bytes, s);
}

int ivf_search_finish(const char* kind, SearchStats& st, const IvfLists& L, int device, hipStream_t s, int64_t nq, int k,
                      float* D, const void* Dd, int64_t* I, const void* Id, int out_mem, int64_t ntotal) {
    HIP_TRY(hipMemcpyAsync(st.pin_cnt, st.cnt, 12, hipMemcpyDeviceToHost, s));
    st.counts_pending = true;
    if (out_mem != FX_MEM_HOST) return FX_OK;
    HIP_TRY(hipMemcpyAsync(D, Dd, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(I, Id, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s));
    if (const int rc = st.read_counts(device, s, L.quant); rc != FX_OK) return rc;
    if (st.last_dropped == 0 && st.last_bad_probe == 0) return FX_OK;
    return set_err(FX_E_INTEGRITY,
                   "%s search: %lld candidate row ids outside [0, %lld) were dropped, %lld probed list numbers lay "
                   "outside [0, %lld)",
                   kind, (long long)st.last_dropped, (long long)ntotal, (long long)st.last_bad_probe, (long long)L.nlist);
}

}  // namespace fx

namespace {

int regroup(FxIvf* v) {
    FxIndex* p = v->pay;
    const IvfRows rows{p->ntotal, p->cap_rows, p->row_bytes, p->codes, p->norms, p->idm.labels, v->row_list};
    return ivf_regroup("ivf", *v, rows, false, v->bad, p->stream());
}

// buf holds at least `want` bytes, its first `keep` bytes carried over
hipError_t grow_keep(DevBuf& buf, size_t want, size_t keep, hipStream_t s) {
    if (want <= buf.bytes) return hipSuccess;
    DevBuf nb;
    hipError_t e = nb.ensure(std::max(want, buf.bytes + buf.bytes / 2));
    if (e != hipSuccess) return e;
    if (buf.p && keep > 0) e = hipMemcpyAsync(nb.p, buf.p, keep, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // (work in flight still reads the old buffer)
    if (e != hipSuccess) return e;
    buf.swap(nb);
    return hipSuccess;
}

}  // namespace

extern "C" {

int fx_ivf_create(FxIndex* quantizer, int d, int64_t nlist, int storage_dtype, int metric, FxIvf** out) {
    if (!out) return set_err(FX_E_ARG, "null out");
    *out = nullptr;
    if (nlist < 1) return set_err(FX_E_ARG, "ivf: nlist must be positive (got %lld)", (long long)nlist);
    if (nlist >= (int64_t)INT32_MAX) return set_err(FX_E_UNSUPPORTED, "ivf: more than 2^31-2 lists");
    if (!quantizer) return set_err(FX_E_ARG, "ivf: null quantizer");
    if (quantizer->d != d)
        return set_err(FX_E_ARG, "ivf: the quantizer has d = %d, the index d = %d", quantizer->d, d);
    if (quantizer->has_ids) return set_err(FX_E_ARG, "ivf: the quantizer carries labels (add_with_ids)");
    if (quantizer->id_offset != 0)
        return set_err(FX_E_ARG, "ivf: the quantizer has id offset %lld", (long long)quantizer->id_offset);
    FxIndex* pay = nullptr;
    if (const int rc = fx_index_create(d, storage_dtype, metric, quantizer->device, &pay); rc != FX_OK) return rc;
    FxIvf* v = new FxIvf();
    v->quant = quantizer;
    v->pay = pay;
    v->device = pay->device;
    v->nlist = nlist;
    v->h_off.assign((size_t)nlist + 1, 0);
    DeviceGuard g(pay->device);
    hipError_t e = v->list_off.ensure((size_t)(nlist + 1) * 4);
    if (e == hipSuccess) e = hipMemset(v->list_off, 0, (size_t)(nlist + 1) * 4);
    if (e == hipSuccess) e = v->max_rows.ensure(16);
    if (e == hipSuccess) e = v->bad.ensure(8);
    if (e == hipSuccess) e = hipMemset(v->bad, 0, 8);
    if (e == hipSuccess) e = v->init_counts();
    if (e != hipSuccess) {
        fx_ivf_free(v);
        return set_err(FX_E_HIP, "ivf init: %s", hipGetErrorString(e));
    }
    *out = v;
    return FX_OK;
}

void fx_ivf_free(FxIvf* v) {
    if (!v) return;
    FxIndex* pay = v->pay;
    {
        DeviceGuard g(pay->device);
        (void)hipStreamSynchronize(pay->stream());
        v->destroy_events();
        v->pay = nullptr;
        delete v;  // its buffers, with the device current
    }
    fx_index_free(pay);
}

int fx_ivf_add(FxIvf* v, int64_t n, const void* x, int x_dtype, int x_mem, const int64_t* ids, int ids_mem) {
    // (the handle last: the other checks are then reachable without a device)
    if (const int rc = check_rows(n, x_dtype, x_mem); rc != FX_OK) return rc;
    if (ids && !valid_mem(ids_mem)) return set_err(FX_E_ARG, "bad ids_mem %d", ids_mem);
    if (!v) return set_err(FX_E_ARG, "null ivf index");
    if (n == 0) return FX_OK;
    if (!x) return set_err(FX_E_ARG, "null x");
    std::lock_guard<std::mutex> lk(v->mu);
    if (const int rc = ivf_quant_trained(*v, "ivf add"); rc != FX_OK) return rc;
    FxIndex* p = v->pay;
    if (const int rc = ivf_add_mode(*v, p->ntotal, ids); rc != FX_OK) return rc;
    if (p->ntotal + n + TILE_R >= (int64_t)INT32_MAX)
        return set_err(FX_E_UNSUPPORTED, "ivf: more than 2^31-1 rows");
    DeviceGuard g(p->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", p->device);
    hipStream_t s = p->stream();
    // a list's last tile may start up to 127 rows before the list's end: the
    // arrays hold a whole tile past the last row
    if (const int rc = fx_index_reserve(p, p->ntotal + n + TILE_R); rc != FX_OK) return rc;
    HIP_TRY(grow_keep(v->row_list, (size_t)p->cap_rows * 4, (size_t)p->ntotal * 4, s));

    // the new rows' lists: the quantizer's k = 1 search, chunk by chunk
    const int64_t rowb = (int64_t)p->d * dtype_size(x_dtype);
    const int64_t chunk = std::min<int64_t>(n, v->quant->opt.kmeans_chunk > 0 ? v->quant->opt.kmeans_chunk
                                                                               : (int)KMEANS_CHUNK_DEFAULT);
    HIP_TRY(v->assign.ensure((size_t)chunk * 12));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t nr = std::min(chunk, n - r0);
        int64_t* a = (int64_t*)v->assign.p;
        float* dd = (float*)((char*)v->assign.p + (size_t)chunk * 8);
        {
            BorrowQuant bq(v->quant, s);
            HIP_TRY(bq.begin());
            const int rc = do_search(v->quant, nr, (const char*)x + r0 * rowb, x_dtype, x_mem, 1, dd, a, FX_MEM_DEVICE);
            if (rc != FX_OK) return rc;
        }
        HIP_TRY(launch_ivf_record(a, nr, v->nlist, v->row_list + p->ntotal + r0, v->bad, s));
    }
    // rows and labels to the payload's tail
    const int64_t* dids = ids;
    int dmem = ids_mem;
    if (!ids) {
        HIP_TRY(v->ids.ensure((size_t)n * 8));
        HIP_TRY(launch_ivf_iota((int64_t*)v->ids.p, n, p->ntotal, s));
        dids = (const int64_t*)v->ids.p;
        dmem = FX_MEM_DEVICE;
    }
    const bool first = p->ntotal == 0;
    if (const int rc = fx_index_add_with_ids(p, n, x, x_dtype, x_mem, dids, dmem); rc != FX_OK) return rc;
    if (first) v->sequential = ids == nullptr;
    v->dirty = true;
    if (x_mem == FX_MEM_HOST) {  // a host call waits for its work: its skipped rows are known now
        int64_t bad = 0;
        if (const int rc = ivf_read_bad(v->bad, s, &bad); rc != FX_OK) return rc;
        if (bad > 0) return ivf_bad_error("ivf", bad, v->nlist);
    }
    return FX_OK;
}

int fx_ivf_search(FxIvf* v, int64_t nq, const void* q, int q_dtype, int q_mem, int k, int nprobe, float* D, int64_t* I,
                  int out_mem) {
    if (const int rc = ivf_search_args("ivf", nq, k, nprobe, q_dtype, q_mem, out_mem); rc != FX_OK) return rc;
    if (!v) return set_err(FX_E_ARG, "null ivf index");
    std::lock_guard<std::mutex> lk(v->mu);
    if (const int rc = ivf_quant_trained(*v, "ivf search"); rc != FX_OK) return rc;
    if (nq == 0) return FX_OK;
    if (!q || !D || !I) return set_err(FX_E_ARG, "null buffer");
    int np = 0;
    if (const int rc = ivf_probes("ivf", *v, nq, nprobe, &np); rc != FX_OK) return rc;
    FxIndex* p = v->pay;
    DeviceGuard g(p->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", p->device);
    if (const int rc = regroup(v); rc != FX_OK) return rc;
    // (an earlier device search's counts, if nobody asked for them, give way to this search's)
    v->clear_counts();
    if (p->ntotal == 0) return fill_missing(p, nq, k, D, I, out_mem);

    hipStream_t s = p->stream();
    const IvfPlan P = plan_ivf(nq, np, v->nlist, v->max_list_rows, p->ntotal, k, p->row_bytes);
    const int qes = dtype_size(q_dtype);
    const void* qdev = nullptr;
    HIP_TRY(stage_in(s, v->qin, q, (size_t)nq * p->d * qes, q_mem, &qdev));
    void *Dd = D, *Id = I;
    HIP_TRY(out_buf(v->outD, D, (size_t)nq * k * 4, out_mem, &Dd));
    HIP_TRY(out_buf(v->outI, I, (size_t)nq * k * 8, out_mem, &Id));
    HIP_TRY(hipMemsetAsync(v->cnt, 0, 16, s));
    const int C = P.chunks, slots = P.slots;
    const bool fused = P.path == IVF_PATH_FUSED;
    const int64_t qb_max = std::min(P.q_batch, nq);
    const int64_t nq_pad_max = round_up(qb_max, QPAD);
    HIP_TRY(ivf_search_workspace(*v, P, nq, np, k));
    HIP_TRY(v->qb.f32.ensure((size_t)nq_pad_max * p->kdim * 4));
    if (fused) {
        HIP_TRY(v->qb.op.ensure((size_t)nq_pad_max * p->row_bytes));
        HIP_TRY(v->qb.eps.ensure((size_t)qb_max * 4));
        HIP_TRY(v->qb.rho.ensure((size_t)qb_max * 4));
        HIP_TRY(v->qb.shift.ensure((size_t)qb_max * 8));
    }
    int* n_flag = (int*)v->flag.p;

    for (int64_t q0 = 0; q0 < nq; q0 += qb_max) {
        const int64_t qb = std::min(qb_max, nq - q0);
        const void* qp = (const char*)qdev + (size_t)q0 * p->d * qes;
        hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        HIP_TRY(v->begin_pass(ev, 5, s));
        // 1. coarse: the quantizer's exact top-np search names the probed lists
        if (const int rc = ivf_coarse(*v, s, qb, qp, q_dtype, np); rc != FX_OK) return rc;
        HIP_TRY(v->mark(ev[1], s));
        IvfExact ex{};
        ex.codes = p->codes;
        ex.row_bytes = p->row_bytes;
        ex.kdim = p->kdim;
        ex.list_off = v->list_off;
        ex.nlist = v->nlist;
        ex.coarse = (const int64_t*)v->coarse_i.p;
        ex.np = np;
        ex.C = C;
        ex.qf32 = (const float*)v->qb.f32.p;
        ex.n_flag = n_flag;
        ex.k = k;
        ex.cd = (float*)v->cand_d.p;
        ex.ci = (int*)v->cand_i.p;
        ex.labels = p->idm.labels;
        ex.D = (float*)Dd + q0 * k;
        ex.I = (int64_t*)Id + q0 * k;
        if (!fused) {
            // the exact path for the whole pass: every query "flagged"
            HIP_TRY(launch_f32_queries(qp, q_dtype, qb, p->d, p->kdim, (float*)v->qb.f32.p, s));
            HIP_TRY(launch_ivf_count_bad(ex.coarse, qb * np, v->nlist, v->cnt + 2, s));
            HIP_TRY(launch_ivf_flag_all(n_flag, qb, s));
            HIP_TRY(v->mark(ev[2], s));
            HIP_TRY(launch_ivf_exact(p->dtype, p->metric, ex, s));
            HIP_TRY(v->mark(ev[3], s));  // (the exact scan is this path's "list scan"; it has no refine)
            HIP_TRY(v->mark(ev[4], s));
            continue;
        }
        // 2. the pass's (query, list) pairs grouped by list
        HIP_TRY(ivf_pairs(*v, v->cnt + 2, qb, np, s));
        // query operands over the stored rows with plain norms (no image), as range_search prepares them
        const int64_t nq_pad = round_up(qb, QPAD);
        PrepParams pp{};
        base_prep(p, v->qb, qp, q_dtype, qb, nq_pad, p->dtype, pp);
        pp.zero[1] = n_flag;
        HIP_TRY(launch_prep_queries(pp, s));
        // 3. the list scan; slots no block writes hold id -1
        HIP_TRY(hipMemsetAsync(v->cand_i.p, 0xff, (size_t)qb * slots * KP * 4, s));
        IvfScan sc{};
        sc.codes = p->codes;
        sc.norms = p->norms;
        sc.row_bytes = p->row_bytes;
        sc.list_off = v->list_off;
        sc.nlist = v->nlist;
        sc.qop = (const char*)v->qb.op.p;
        sc.np = np;
        sc.C = C;
        sc.sorted = (uint64_t*)v->psorted.p;
        sc.seg = (int*)v->seg.p;
        sc.gbase = (int*)v->gbase.p;
        sc.cand_d = (float*)v->cand_d.p;
        sc.cand_i = (int*)v->cand_i.p;
        sc.grid = (qb * np / TILE_Q + std::min<int64_t>(v->nlist, qb * np)) * C;
        HIP_TRY(v->mark(ev[2], s));
        HIP_TRY(launch_ivf_scan(p->dtype, p->metric, sc, s));
        HIP_TRY(v->mark(ev[3], s));
#ifdef FX_DIAG
        // FX_IVF_CAND (read when the index was created): the pass's scan lists, probed lists and list
        // offsets appended to the file, before the refine reads the lists and the exact scan writes over them:
        //   cand_d, cand_i [qb][slots][KP] | coarse [qb][np] i64 | list_off [nlist + 1]
        if (!p->opt.ivf_cand.empty()) {
            const std::string& path = p->opt.ivf_cand;
            HIP_TRY(hipStreamSynchronize(s));
            HIP_TRY(dump_device<float>(path, sc.cand_d, (size_t)qb * slots * KP));
            HIP_TRY(dump_device<int>(path, sc.cand_i, (size_t)qb * slots * KP));
            HIP_TRY(dump_device<int64_t>(path, ex.coarse, (size_t)qb * np));
            HIP_TRY(dump_device<int>(path, v->list_off, (size_t)v->nlist + 1));
        }
#endif
        // 4. refine + certification over the query's slots (one "query tile" per query)
        RefineParams rp{};
        rp.cand_d = sc.cand_d;
        rp.cand_i = sc.cand_i;
        rp.splits = slots;
        rp.qt = 1;
        rp.nq = qb;
        rp.ntotal = p->ntotal;
        rp.k = k;
        rp.codes = p->codes;
        rp.row_bytes = p->row_bytes;
        rp.kdim = p->kdim;
        rp.qf32 = pp.qf32;
        rp.qeps = pp.qeps;
        rp.qrho = pp.qrho;
        rp.qshift = pp.qshift;
        rp.id_offset = 0;
        rp.labels = p->idm.labels;
        rp.D = ex.D;
        rp.I = ex.I;
        rp.n_flag = n_flag;
        rp.flag_list = n_flag + 1;
        rp.n_drop = v->cnt;
        rp.prefetch = qb <= 256 ? 4 : 1;
        rp.k1 = 0;
        rp.force_fb = v->quant->opt.force_fallback != 0;  // (the diagnostic build's hook, set on the quantizer)
        rp.gtau = nullptr;
        rp.wg = 0;
        HIP_TRY(launch_refine(p->dtype, p->metric, rp, s));
        // 5. the flagged queries' exact lists (device-gated; the candidate buffers are free again)
        HIP_TRY(launch_ivf_exact(p->dtype, p->metric, ex, s));
        HIP_TRY(launch_ivf_accum(v->cnt + 1, n_flag, s));
        HIP_TRY(v->mark(ev[4], s));
    }
    return ivf_search_finish("ivf", *v, *v, p->device, s, nq, k, D, Dd, I, Id, out_mem, p->ntotal);
}

int fx_ivf_reset(FxIvf* v) {
    if (!v) return set_err(FX_E_ARG, "null ivf index");
    std::lock_guard<std::mutex> lk(v->mu);
    if (const int rc = fx_index_reset(v->pay); rc != FX_OK) return rc;
    DeviceGuard g(v->pay->device);
    HIP_TRY(hipMemset(v->list_off, 0, (size_t)(v->nlist + 1) * 4));
    HIP_TRY(hipMemset(v->bad, 0, 8));
    v->h_off.assign((size_t)v->nlist + 1, 0);
    v->max_list_rows = 0;
    v->dirty = false;
    v->sequential = false;
    return FX_OK;
}

int fx_ivf_ntotal(const FxIvf* v, int64_t* out) {
    if (!v || !out) return set_err(FX_E_ARG, "null argument");
    *out = v->pay->ntotal;
    return FX_OK;
}

int fx_ivf_list_sizes(FxIvf* v, int64_t* out) { return ivf_list_sizes(v, regroup, out); }

int fx_ivf_list_ids(FxIvf* v, int64_t list, int64_t* out, int64_t cap, int64_t* n) {
    if (!v) return set_err(FX_E_ARG, "null argument");
    return ivf_list_ids(v, "ivf", regroup, v->pay->idm.labels, list, out, cap, n);
}

int fx_ivf_set_stream(FxIvf* v, void* stream) {
    if (!v) return set_err(FX_E_ARG, "null ivf index");
    std::lock_guard<std::mutex> lk(v->mu);
    return fx_index_set_stream(v->pay, stream);
}

int fx_ivf_last_counts(FxIvf* v, int64_t* fallbacks, int64_t* exact_fallbacks, int64_t* dropped) {
    return handle_last_counts(v, v ? v->quant : nullptr, fallbacks, exact_fallbacks, dropped);
}

int fx_ivf_profile(FxIvf* v, int enable) { return handle_profile(v, "ivf", enable); }

int fx_ivf_profile_read(FxIvf* v, double* coarse_ms, double* pairs_ms, double* scan_ms, double* refine_ms,
                        int64_t* passes) {
    double* const ms[] = {coarse_ms, pairs_ms, scan_ms, refine_ms};
    return handle_profile_read(v, ms, passes);
}

int fx_ivf_last_plan(FxIvf* v, int* path, int* chunks, int* slots, int64_t* q_batch, int64_t* grid) {
    return ivf_last_plan(v, path, chunks, slots, q_batch, grid);
}

}  // extern "C"

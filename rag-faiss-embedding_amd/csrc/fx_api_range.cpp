// fx_api_range.cpp -- range_search (fx_range.hip).
#include "fx_host.h"
#include "fx_plan.h"

using namespace fx;

namespace {

static int range_store_empty(FxIndex* h, int64_t nq, int64_t* lims) {
    // no row can qualify: all-zero lims on the host and on the device
    HIP_TRY(h->rg.lims.ensure((size_t)(nq + 1) * 8));
    HIP_TRY(hipMemsetAsync(h->rg.lims.p, 0, (size_t)(nq + 1) * 8, h->stream()));
    HIP_TRY(hipStreamSynchronize(h->stream()));
    std::fill(lims, lims + nq + 1, (int64_t)0);
    h->rg.nq = nq;
    h->rg.total = 0;
    return FX_OK;
}

// DevBuf growth of the range path: an allocation failure is FX_E_OOM
#define RG_ALLOC(buf, want)                                                                          \
    do {                                                                                             \
        if ((buf).ensure(want) != hipSuccess) {                                                      \
            (void)hipGetLastError();                                                                 \
            return set_err(FX_E_OOM, "range_search: cannot allocate %zu bytes (%s)", (size_t)(want), #buf); \
        }                                                                                            \
    } while (0)

}  // namespace

extern "C" {

int fx_index_range_search(FxIndex* h, int64_t nq, const void* q, int q_dtype, int q_mem, float radius,
                          int64_t* lims) {
    if (radius != radius) return set_err(FX_E_ARG, "range_search: radius is NaN");
    if (!h) return set_err(FX_E_ARG, "null index");
    if (nq < 0) return set_err(FX_E_ARG, "negative nq");
    if (nq >= (int64_t)INT32_MAX) return set_err(FX_E_UNSUPPORTED, "range_search: more than 2^31-1 queries per call");
    if (!check_dtype(q_dtype)) return set_err(FX_E_ARG, "bad query dtype %d", q_dtype);
    if (!lims) return set_err(FX_E_ARG, "null lims");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    {   // the counts of a device-resident search still in flight are read first:
        // this call reuses the dropped-ids word
        const int rc = read_counts(h);
        if (rc != FX_OK) return rc;
    }
    h->rg.nq = -1;
    h->rg.total = 0;
    h->rg.cands = 0;
    h->rg.passes = 0;
    if (nq == 0) {
        lims[0] = 0;
        h->rg.nq = 0;
        return FX_OK;
    }
    if (!q) return set_err(FX_E_ARG, "null buffer");
    // L2 distances are >= 0 and the test is strict: radius <= 0 takes no row
    if (h->ntotal == 0 || (h->metric == L2 && radius <= 0.0f)) return range_store_empty(h, nq, lims);

    hipStream_t s = h->stream();
    const size_t qb = (size_t)nq * h->d * dtype_size(q_dtype);
    if (q_mem == FX_MEM_HOST) RG_ALLOC(h->rg.qin, qb);
    const void* qdev = nullptr;
    HIP_TRY(stage_in(h->stream(), h->rg.qin, q, qb, q_mem, &qdev));
    const int64_t nq_pad = round_up(nq, QPAD);
    RG_ALLOC(h->rg.f32, (size_t)nq_pad * h->kdim * 4);
    RG_ALLOC(h->rg.op, (size_t)nq_pad * h->row_bytes);
    RG_ALLOC(h->rg.eps, (size_t)nq * 4);
    RG_ALLOC(h->rg.rho, (size_t)nq * 4);
    RG_ALLOC(h->rg.shift, (size_t)nq * 8);
    RG_ALLOC(h->rg.thr, (size_t)nq * 4);
    RG_ALLOC(h->rg.cnt, 8);
    RG_ALLOC(h->rg.lims, (size_t)(nq + 1) * 8);
    const uint64_t want_cap = h->opt.range_cap > 0 ? (uint64_t)h->opt.range_cap : (uint64_t)RANGE_CAP_DEFAULT;
    RG_ALLOC(h->rg.cand, (size_t)want_cap * 8);

    // query preparation in its no-image mode: the operand of the stored rows'
    // dtype, uncentred, bound terms against max |y|^2
    PrepParams pp{};
    base_prep(h, h->rg, qdev, q_dtype, nq, nq_pad, h->dtype, pp);
    pp.zero[0] = h->dev_drop;
    HIP_TRY(launch_prep_queries(pp, s));
    HIP_TRY(launch_range_thr(nq, h->metric, radius, pp.qeps, pp.qrho, pp.qshift, (float*)h->rg.thr.p, s));

    ScanParams sp{};
    base_scan(h, IMG_NONE, h->rg, nq, sp);
    plan_range_scan(h->shape(), nq, sp);

    // the scan; when it counted more candidates than the buffer holds, the
    // buffer grows to the count and the scan runs once more (the count does
    // not depend on the capacity, so the second pass fits)
    uint64_t count = 0;
    for (int pass = 1; pass <= 2; ++pass) {
        const uint64_t cap = h->rg.cand.bytes / 8;
        HIP_TRY(hipMemsetAsync(h->rg.cnt.p, 0, 8, s));
        HIP_TRY(launch_range_scan(h->dtype, h->metric, sp, (const float*)h->rg.thr.p, (uint64_t*)h->rg.cand.p, cap,
                                  (uint64_t*)h->rg.cnt.p, s));
        HIP_TRY(hipMemcpyAsync(&count, h->rg.cnt.p, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        h->rg.passes = pass;
        if (count <= cap) break;
        if (pass == 2)
            return set_err(FX_E_INTEGRITY, "range_search: the second scan pass counted %llu candidates for %llu slots",
                           (unsigned long long)count, (unsigned long long)cap);
        if (count > (uint64_t)INT32_MAX)
            return set_err(FX_E_UNSUPPORTED, "range_search: %llu candidate pairs in one call (limit 2^31-1): "
                           "search fewer queries per call", (unsigned long long)count);
        RG_ALLOC(h->rg.cand, (size_t)count * 8);
    }
    h->rg.cands = (int64_t)count;
    if (count == 0) return range_store_empty(h, nq, lims);

    RangeFinish f{};
    f.n = (int64_t)count;
    HIP_TRY(range_sort_temp_bytes(f.n, nq, &f.temp_bytes));
    RG_ALLOC(h->rg.dist, (size_t)count * 4);
    RG_ALLOC(h->rg.sorted, (size_t)count * 8);
    RG_ALLOC(h->rg.temp, std::max<size_t>(f.temp_bytes, 16));
    RG_ALLOC(h->rg.D, (size_t)count * 4);
    RG_ALLOC(h->rg.I, (size_t)count * 8);
    f.words = (uint64_t*)h->rg.cand.p;
    f.codes = h->codes;
    f.row_bytes = h->row_bytes;
    f.kdim = h->kdim;
    f.st_dt = h->dtype;
    f.metric = h->metric;
    f.ntotal = h->ntotal;
    f.qf32 = pp.qf32;
    f.nq = nq;
    f.radius = radius;
    f.id_offset = h->id_offset;
    f.labels = h->label_ptr();
    f.dist = (float*)h->rg.dist.p;
    f.sorted = (uint64_t*)h->rg.sorted.p;
    f.temp = h->rg.temp.p;
    f.n_drop = h->dev_drop;
    f.lims = (int64_t*)h->rg.lims.p;
    f.D = (float*)h->rg.D.p;
    f.I = (int64_t*)h->rg.I.p;
    HIP_TRY(launch_range_finish(f, s));
    int dropped = 0;
    HIP_TRY(hipMemcpyAsync(lims, f.lims, (size_t)(nq + 1) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&dropped, h->dev_drop, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    h->last_dropped = dropped;
    if (dropped > 0) return integrity_error(h);
    h->rg.nq = nq;
    h->rg.total = lims[nq];
    return FX_OK;
}
#undef RG_ALLOC

int fx_index_range_result(FxIndex* h, float* D, int64_t* I, int out_mem) {
    if (!h) return set_err(FX_E_ARG, "null index");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->rg.nq < 0) return set_err(FX_E_ARG, "range_result: no range search result is stored");
    if (h->rg.total == 0) return FX_OK;
    if (!D || !I) return set_err(FX_E_ARG, "null buffer");
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    const hipMemcpyKind kind = out_mem == FX_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    HIP_TRY(hipMemcpyAsync(D, h->rg.D.p, (size_t)h->rg.total * 4, kind, s));
    HIP_TRY(hipMemcpyAsync(I, h->rg.I.p, (size_t)h->rg.total * 8, kind, s));
    if (out_mem == FX_MEM_HOST) HIP_TRY(hipStreamSynchronize(s));
    return FX_OK;
}

int fx_index_last_range_stats(FxIndex* h, int64_t* candidates, int* passes) {
    if (!h || !candidates || !passes) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *candidates = h->rg.cands;
    *passes = h->rg.passes;
    return FX_OK;
}

}  // extern "C"

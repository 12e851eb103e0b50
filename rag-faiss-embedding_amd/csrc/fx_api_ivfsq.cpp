// fx_api_ivfsq.cpp -- inverted file over 8-bit codes (fx_ivfsq.hip): fx_ivfsq_create / _train / _add /
// _search and the accessors.  The index owns its payload (codes, n_c, labels, the rows' lists) and its
// tables; the lists are the inverted file's (the quantizer's k = 1 search, the regroup of fx_ivf.hip),
// the rows the scalar quantizer's (fx_sq.hip's min / max training and encoder, fed with residuals).
#include "fx_host.h"
#include "fx_plan.h"

using namespace fx;

namespace {

constexpr int QT_8BIT = 0, QT_8BIT_UNIFORM = 2;
// rows per chunk of train / add: the quantizer's chunk, and at most 256 MiB of fp32 residuals
int64_t ivfsq_chunk(const FxIvfSq* v, int64_t n) {
    const int64_t kc = v->quant->opt.kmeans_chunk > 0 ? v->quant->opt.kmeans_chunk : (int)KMEANS_CHUNK_DEFAULT;
    const int64_t rc = std::max<int64_t>(1, (256ll << 20) / ((int64_t)v->d * 4));
    return std::max<int64_t>(1, std::min(n, std::min(kc, rc)));
}

hipError_t ivfsq_stage_in(FxIvfSq* v, DevBuf& buf, const void* src, size_t bytes, int mem, const void** dev) {
    if (mem == FX_MEM_DEVICE) {
        *dev = src;
        return hipSuccess;
    }
    hipError_t e = buf.ensure(std::max<size_t>(bytes, 16));
    if (e != hipSuccess) return e;
    *dev = buf.p;
    return hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, v->stream());
}

int ivfsq_quant_trained(const FxIvfSq* v, const char* who) {
    if (v->quant->ntotal != v->nlist)
        return set_err(FX_E_ARG, "%s: the index is not trained (the quantizer holds %lld of %lld centroids)", who,
                       (long long)v->quant->ntotal, (long long)v->nlist);
    return FX_OK;
}

int ivfsq_need_trained(const FxIvfSq* v, const char* who) {
    if (const int rc = ivfsq_quant_trained(v, who); rc != FX_OK) return rc;
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

// capacity for n rows and a whole tile past the last one (a list's last tile may start up to 127 rows
// before the list's end); new rows hold code 0 and n_c = 0 (the scan masks rows by row number)
hipError_t ivfsq_grow(FxIvfSq* v, int64_t n) {
    const int64_t want = round_up(n, TILE_R) + TILE_R;
    if (want <= v->cap_rows) return hipSuccess;
    const int64_t cap = std::max(want, round_up(v->cap_rows + v->cap_rows / 2, TILE_R));
    hipStream_t s = v->stream();
    DevBuf codes, nc, labels, rl;
    hipError_t e = codes.ensure((size_t)cap * v->row_bytes);
    if (e == hipSuccess) e = nc.ensure((size_t)cap * 4);
    if (e == hipSuccess) e = labels.ensure((size_t)cap * 8);
    if (e == hipSuccess) e = rl.ensure((size_t)cap * 4);
    if (e == hipSuccess) e = hipMemsetAsync(codes.p, 0, (size_t)cap * v->row_bytes, s);
    if (e == hipSuccess) e = hipMemsetAsync(nc.p, 0, (size_t)cap * 4, s);
    if (e == hipSuccess && v->ntotal > 0) {
        const size_t n0 = (size_t)v->ntotal;
        e = hipMemcpyAsync(codes.p, v->codes.p, n0 * v->row_bytes, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(nc.p, v->nc.p, n0 * 4, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(labels.p, v->labels.p, n0 * 8, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(rl.p, v->row_list.p, n0 * 4, hipMemcpyDeviceToDevice, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // (work in flight still reads the old buffers)
    if (e != hipSuccess) return e;
    v->codes.swap(codes);
    v->nc.swap(nc);
    v->labels.swap(labels);
    v->row_list.swap(rl);
    v->cap_rows = cap;
    return hipSuccess;
}

int ivfsq_bad_error(int64_t bad, int64_t nlist) {
    return set_err(FX_E_INTEGRITY, "ivfsq: %lld rows were assigned outside [0, %lld) and belong to no list",
                   (long long)bad, (long long)nlist);
}

// the skipped-assignment count since the last read, then 0 again (synchronises)
int ivfsq_read_bad(FxIvfSq* v, int64_t* out) {
    hipStream_t s = v->stream();
    unsigned long long bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, v->bad + 1, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(v->bad + 1, 0, 8, s));
    HIP_TRY(hipStreamSynchronize(s));
    *out = (int64_t)bad;
    return FX_OK;
}

// the payload in list order (a no-op unless rows were added since): fx_api_ivf.cpp's regroup over
// this index's buffers, n_c in the place of the norms
int ivfsq_regroup(FxIvfSq* v) {
    if (!v->dirty) return FX_OK;
    hipStream_t s = v->stream();
    const int64_t n = v->ntotal;
    v->h_off.assign((size_t)v->nlist + 1, 0);
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(v->list_off, 0, (size_t)(v->nlist + 1) * 4, s));
        v->max_list_rows = 0;
        v->dirty = false;
        return FX_OK;
    }
    HIP_TRY(v->codes_alt.ensure((size_t)v->cap_rows * v->row_bytes));
    HIP_TRY(v->nc_alt.ensure((size_t)v->cap_rows * 4));
    HIP_TRY(v->labels_alt.ensure((size_t)v->cap_rows * 8));
    HIP_TRY(v->row_list_alt.ensure((size_t)v->cap_rows * 4));
    // (the rows past n of the buffers that come in: code 0, n_c = 0, as ivfsq_grow leaves them)
    HIP_TRY(hipMemsetAsync(v->codes_alt.p, 0, v->codes_alt.bytes, s));
    HIP_TRY(hipMemsetAsync(v->nc_alt.p, 0, v->nc_alt.bytes, s));
    size_t ws = 0;
    HIP_TRY(ivf_regroup_bytes(n, v->nlist, &ws));
    HIP_TRY(v->rws.ensure(ws));
    IvfRegroup r{};
    r.n = n;
    r.nlist = v->nlist;
    r.row_bytes = v->row_bytes;
    r.codes = v->codes;
    r.norms = v->nc;
    r.labels = v->labels;
    r.row_list = v->row_list;
    r.dst_codes = v->codes_alt;
    r.dst_norms = v->nc_alt;
    r.dst_labels = v->labels_alt;
    r.dst_row_list = v->row_list_alt;
    r.list_off = v->list_off;
    r.max_rows = v->max_rows;
    HIP_TRY(launch_ivf_regroup(r, v->rws.p, v->rws.bytes, s));
    int max_rows = 0;
    HIP_TRY(hipMemcpyAsync(&max_rows, v->max_rows, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(v->h_off.data(), v->list_off, (size_t)(v->nlist + 1) * 4, hipMemcpyDeviceToHost, s));
    int64_t bad = 0;
    if (const int rc = ivfsq_read_bad(v, &bad); rc != FX_OK) return rc;
    // (the stream is idle: nothing reads the buffers that go out)
    v->codes.swap(v->codes_alt);
    v->nc.swap(v->nc_alt);
    v->labels.swap(v->labels_alt);
    v->row_list.swap(v->row_list_alt);
    // the second copy goes again: device memory is back at one payload
    v->codes_alt.release();
    v->nc_alt.release();
    v->labels_alt.release();
    v->row_list_alt.release();
    v->max_list_rows = max_rows;
    v->dirty = false;
    if (bad > 0) return ivfsq_bad_error(bad, v->nlist);
    return FX_OK;
}

int ivfsq_read_counts(FxIvfSq* v) {
    if (v->counts_pending) {
        DeviceGuard g(v->device);
        HIP_TRY(hipStreamSynchronize(v->stream()));
        v->last_dropped = v->pin_cnt[0];
        v->last_fallbacks = v->pin_cnt[1];
        v->last_bad_probe = v->pin_cnt[2];
        v->counts_pending = false;
        // the borrowed coarse search's own integrity count (of the last pass; its copies ran on this stream)
        std::lock_guard<std::mutex> ql(v->quant->mu);
        if (const int rc = read_counts(v->quant); rc != FX_OK) return rc;
    }
    return FX_OK;
}

int ivfsq_integrity(const FxIvfSq* v) {
    return set_err(FX_E_INTEGRITY,
                   "ivfsq search: %lld candidate row ids outside [0, %lld) were dropped, %lld probed list numbers lay "
                   "outside [0, %lld)",
                   (long long)v->last_dropped, (long long)v->ntotal, (long long)v->last_bad_probe, (long long)v->nlist);
}

// D / I of a search over an empty index
int ivfsq_fill_missing(FxIvfSq* v, int64_t nq, int k, float* D, int64_t* I, int out_mem) {
    const size_t n = (size_t)nq * k;
    std::vector<float> hd(n, v->metric == L2 ? FLT_MAX : -FLT_MAX);
    std::vector<int64_t> hi(n, -1);
    if (out_mem == FX_MEM_HOST) {
        memcpy(D, hd.data(), n * 4);
        memcpy(I, hi.data(), n * 8);
        return FX_OK;
    }
    hipStream_t s = v->stream();
    HIP_TRY(hipMemcpyAsync(D, hd.data(), n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(I, hi.data(), n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // (the host vectors go out of scope)
    return FX_OK;
}

int ivfsq_check_rows(int64_t n, int x_dtype, int x_mem) {
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (!check_dtype(x_dtype)) return set_err(FX_E_ARG, "bad x dtype %d", x_dtype);
    if (!valid_mem(x_mem)) return set_err(FX_E_ARG, "bad x_mem %d", x_mem);
    return FX_OK;
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
    v->row_bytes = (int)round_up(d, ROW_ALIGN);
    v->h_off.assign((size_t)nlist + 1, 0);
    v->opt.from_env();
    hipError_t e = hipStreamCreateWithFlags(&v->own_stream, hipStreamDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&v->switch_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = v->tables.ensure((size_t)2 * d * 4);
    if (e == hipSuccess) e = v->mm.ensure((size_t)2 * d * 4);
    if (e == hipSuccess) e = v->words.ensure(SQ_WORDS * 4);
    if (e == hipSuccess) e = hipMemset(v->words, 0, SQ_WORDS * 4);
    if (e == hipSuccess) e = v->list_off.ensure((size_t)(nlist + 1) * 4);
    if (e == hipSuccess) e = hipMemset(v->list_off, 0, (size_t)(nlist + 1) * 4);
    if (e == hipSuccess) e = v->max_rows.ensure(16);
    if (e == hipSuccess) e = v->bad.ensure(16);
    if (e == hipSuccess) e = hipMemset(v->bad, 0, 16);
    if (e == hipSuccess) e = v->cnt.ensure(16);
    if (e == hipSuccess) e = hipMemset(v->cnt, 0, 16);
    if (e == hipSuccess) e = v->pin_cnt.ensure(16);
    if (e != hipSuccess) {
        fx_ivfsq_free(v);
        return set_err(FX_E_HIP, "ivfsq init: %s", hipGetErrorString(e));
    }
    v->pin_cnt[0] = v->pin_cnt[1] = v->pin_cnt[2] = 0;
    *out = v;
    return FX_OK;
}

void fx_ivfsq_free(FxIvfSq* v) {
    if (!v) return;
    DeviceGuard g(v->device);
    if (v->own_stream) (void)hipStreamSynchronize(v->own_stream);
    if (v->user_stream) (void)hipStreamSynchronize(v->user_stream);
    for (hipEvent_t e : v->ev) (void)hipEventDestroy(e);
    if (v->switch_ev) (void)hipEventDestroy(v->switch_ev);
    const hipStream_t own = v->own_stream;
    delete v;  // its buffers, with the device current and before the stream goes
    if (own) (void)hipStreamDestroy(own);
}

int fx_ivfsq_train(FxIvfSq* v, int64_t n, const void* x, int x_dtype, int x_mem, int more) {
    // (the handle last: the other checks are then reachable without a device)
    if (const int rc = ivfsq_check_rows(n, x_dtype, x_mem); rc != FX_OK) return rc;
    if (!v) return set_err(FX_E_ARG, "null ivfsq index");
    std::lock_guard<std::mutex> lk(v->mu);
    if (v->ntotal > 0)
        return set_err(FX_E_ARG, "ivfsq train: the index holds %lld rows (reset it first)", (long long)v->ntotal);
    if (const int rc = ivfsq_quant_trained(v, "ivfsq train"); rc != FX_OK) return rc;
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
    const size_t es = dtype_size(x_dtype);
    const int64_t chunk = ivfsq_chunk(v, n);
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t nr = std::min(chunk, n - r0);
        const void* xd = nullptr;
        HIP_TRY(ivfsq_stage_in(v, v->in, (const char*)x + (size_t)r0 * v->d * es, (size_t)nr * v->d * es, x_mem, &xd));
        if (v->by_residual) {
            HIP_TRY(v->tlist.ensure((size_t)nr * 4));
            HIP_TRY(v->resid.ensure((size_t)nr * v->d * 4));
            if (const int rc = ivfsq_assign(v, nr, xd, x_dtype, (int*)v->tlist.p); rc != FX_OK) return rc;
            HIP_TRY(launch_ivfsq_residual(xd, x_dtype, nr, v->d, (const int*)v->tlist.p, v->nlist, v->cent,
                                          (float*)v->resid.p, s));
            HIP_TRY(launch_sq_minmax(v->resid.p, F32, nr, v->d, v->mm, v->bad, s));
        } else {
            HIP_TRY(launch_sq_minmax(xd, x_dtype, nr, v->d, v->mm, v->bad, s));
        }
        if (x_mem == FX_MEM_HOST) HIP_TRY(hipStreamSynchronize(s));  // staging buffer reuse
    }
    if (more) return FX_OK;
    // the one synchronisation of a training: its non-finite and unassigned counts
    unsigned long long bad[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(bad, v->bad, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(v->bad, 0, 16, s));
    HIP_TRY(hipStreamSynchronize(s));
    v->train_open = false;
    if (bad[0] > 0) return set_err(FX_E_ARG, "ivfsq train: %llu non-finite values in the training data", bad[0]);
    if (bad[1] > 0) return ivfsq_bad_error((int64_t)bad[1], v->nlist);
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
    hipStream_t s = v->stream();
    HIP_TRY(hipMemcpyAsync(out, v->tables, (size_t)2 * v->d * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FX_OK;
}

int fx_ivfsq_set_trained(FxIvfSq* v, const float* trained) {
    if (!v || !trained) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(v->mu);
    if (v->ntotal > 0)
        return set_err(FX_E_ARG, "ivfsq set_trained: the index holds %lld rows (reset it first)", (long long)v->ntotal);
    if (const int rc = ivfsq_quant_trained(v, "ivfsq set_trained"); rc != FX_OK) return rc;
    for (int j = 0; j < v->d; ++j)
        if (!std::isfinite(trained[j]) || !std::isfinite(trained[v->d + j]) || trained[v->d + j] < 0.f)
            return set_err(FX_E_ARG, "ivfsq set_trained: dimension %d has vmin = %g, vdiff = %g", j, (double)trained[j],
                           (double)trained[v->d + j]);
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
    if (const int rc = ivfsq_check_rows(n, x_dtype, x_mem); rc != FX_OK) return rc;
    if (ids && !valid_mem(ids_mem)) return set_err(FX_E_ARG, "bad ids_mem %d", ids_mem);
    if (!v) return set_err(FX_E_ARG, "null ivfsq index");
    if (n == 0) return FX_OK;
    if (!x) return set_err(FX_E_ARG, "null x");
    std::lock_guard<std::mutex> lk(v->mu);
    if (const int rc = ivfsq_need_trained(v, "ivfsq add"); rc != FX_OK) return rc;
    if (v->ntotal > 0 && v->sequential && ids)
        return set_err(FX_E_ARG, "add_with_ids not implemented for an index that holds rows without labels");
    if (v->ntotal > 0 && !v->sequential && !ids)
        return set_err(FX_E_ARG, "add does not make sense on an index with labels: use add_with_ids");
    if (v->ntotal + n + 2 * TILE_R >= (int64_t)INT32_MAX)
        return set_err(FX_E_UNSUPPORTED, "ivfsq: more than 2^31-1 rows");
    DeviceGuard g(v->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", v->device);
    hipStream_t s = v->stream();
    HIP_TRY(ivfsq_grow(v, v->ntotal + n));
    const size_t es = dtype_size(x_dtype);
    const int rb = v->row_bytes;
    const int64_t chunk = ivfsq_chunk(v, n);
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t nr = std::min(chunk, n - r0);
        const int64_t row0 = v->ntotal + r0;
        const void* xd = nullptr;
        HIP_TRY(ivfsq_stage_in(v, v->in, (const char*)x + (size_t)r0 * v->d * es, (size_t)nr * v->d * es, x_mem, &xd));
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
        if (x_mem == FX_MEM_HOST) HIP_TRY(hipStreamSynchronize(s));  // staging buffer reuse
    }
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
        if (const int rc = ivfsq_read_bad(v, &bad); rc != FX_OK) return rc;
        if (bad > 0) return ivfsq_bad_error(bad, v->nlist);
    }
    return FX_OK;
}

int fx_ivfsq_search(FxIvfSq* v, int64_t nq, const void* q, int q_dtype, int q_mem, int k, int nprobe, float* D,
                    int64_t* I, int out_mem) {
    if (nq < 0) return set_err(FX_E_ARG, "negative nq");
    if (k < 1) return set_err(FX_E_ARG, "k must be positive (got %d)", k);
    if (nprobe < 1) return set_err(FX_E_ARG, "nprobe must be positive (got %d)", nprobe);
    if (!check_dtype(q_dtype)) return set_err(FX_E_ARG, "bad query dtype %d", q_dtype);
    if (!valid_mem(q_mem) || !valid_mem(out_mem)) return set_err(FX_E_ARG, "bad q_mem / out_mem");
    if (k > FX_MAX_K) return set_err(FX_E_UNSUPPORTED, "ivfsq search: k = %d above FX_MAX_K = %d", k, FX_MAX_K);
    if (!v) return set_err(FX_E_ARG, "null ivfsq index");
    std::lock_guard<std::mutex> lk(v->mu);
    if (const int rc = ivfsq_need_trained(v, "ivfsq search"); rc != FX_OK) return rc;
    if (nq == 0) return FX_OK;
    if (!q || !D || !I) return set_err(FX_E_ARG, "null buffer");
    const int np = (int)std::min<int64_t>(nprobe, v->nlist);
    if (nq * np >= (int64_t)INT32_MAX)
        return set_err(FX_E_UNSUPPORTED, "ivfsq search: nq * nprobe = %lld pairs (limit 2^31-1)", (long long)(nq * np));
    if (np > FX_MAX_K)
        return set_err(FX_E_UNSUPPORTED, "ivfsq search: nprobe = %d above %d (the coarse search's k)", np, FX_MAX_K);
    DeviceGuard g(v->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", v->device);
    if (const int rc = ivfsq_regroup(v); rc != FX_OK) return rc;
    // (an earlier device search's counts, if nobody asked for them, give way to this search's)
    v->counts_pending = false;
    v->last_fallbacks = v->last_dropped = v->last_bad_probe = 0;
    if (v->ntotal == 0) return ivfsq_fill_missing(v, nq, k, D, I, out_mem);

    hipStream_t s = v->stream();
    const int rb = v->row_bytes;
    const IvfSqPlan P = plan_ivfsq(nq, np, v->nlist, v->max_list_rows, v->ntotal, k, rb);
    v->last_plan[0] = P.path;
    v->last_plan[1] = P.chunks;
    v->last_plan[2] = P.slots;
    v->last_qbatch = P.q_batch;
    v->last_grid = P.grid;
    const int qes = dtype_size(q_dtype);
    const void* qdev = nullptr;
    HIP_TRY(ivfsq_stage_in(v, v->qin, q, (size_t)nq * v->d * qes, q_mem, &qdev));
    const bool host_out = out_mem == FX_MEM_HOST;
    float* Dd = D;
    int64_t* Id = I;
    if (host_out) {
        HIP_TRY(v->outD.ensure((size_t)nq * k * 4));
        HIP_TRY(v->outI.ensure((size_t)nq * k * 8));
        Dd = (float*)v->outD.p;
        Id = (int64_t*)v->outI.p;
    }
    HIP_TRY(hipMemsetAsync(v->cnt, 0, 16, s));
    const int C = P.chunks, slots = P.slots;
    const bool fused = P.path == IVF_PATH_FUSED;
    const int64_t qb_max = std::min(P.q_batch, nq);
    const int64_t pad_max = round_up(qb_max * np, TILE_Q);
    HIP_TRY(v->coarse_d.ensure((size_t)qb_max * np * 4));
    HIP_TRY(v->coarse_i.ensure((size_t)qb_max * np * 8));
    HIP_TRY(v->flag.ensure((size_t)(qb_max + 1) * 4));
    HIP_TRY(v->qf32.ensure((size_t)qb_max * rb * 4));
    const size_t ncand = (size_t)qb_max * slots * (fused ? KP : k);
    HIP_TRY(v->cand_d.ensure(ncand * 4));
    HIP_TRY(v->cand_i.ensure(ncand * 4));
    if (fused) {
        HIP_TRY(v->planes.ensure((size_t)SQ_P * pad_max * rb));
        HIP_TRY(v->sigma.ensure((size_t)pad_max * 4));
        HIP_TRY(v->peps.ensure((size_t)pad_max * 4));
        HIP_TRY(v->pshift.ensure((size_t)pad_max * 4));
        HIP_TRY(v->pkeys.ensure((size_t)qb_max * np * 8));
        HIP_TRY(v->psorted.ensure((size_t)qb_max * np * 8));
        HIP_TRY(v->seg.ensure((size_t)(v->nlist + 1) * 4));
        HIP_TRY(v->ngrp.ensure((size_t)(v->nlist + 1) * 4));
        HIP_TRY(v->gbase.ensure((size_t)(v->nlist + 1) * 4));
        // hipCUB's temporaries for every pass size that occurs: full passes and a shorter last one
        size_t tb = 0, tb_last = 0;
        HIP_TRY(ivf_pairs_temp_bytes(qb_max * np, v->nlist, &tb));
        if (nq % qb_max != 0) HIP_TRY(ivf_pairs_temp_bytes((nq % qb_max) * np, v->nlist, &tb_last));
        HIP_TRY(v->ptemp.ensure(std::max<size_t>(std::max(tb, tb_last), 16)));
    }
    int* n_flag = (int*)v->flag.p;
    const float* cent = v->by_residual ? (const float*)v->cent : nullptr;

    for (int64_t q0 = 0; q0 < nq; q0 += qb_max) {
        const int64_t qb = std::min(qb_max, nq - q0);
        const void* qp = (const char*)qdev + (size_t)q0 * v->d * qes;
        hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        if (v->profile) {
            for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
            v->ev.insert(v->ev.end(), ev, ev + 5);
            HIP_TRY(hipEventRecord(ev[0], s));
        }
        // 1. coarse: the quantizer's exact top-np search names the probed lists
        {
            BorrowQuant bq(v->quant, s);
            HIP_TRY(bq.begin());
            const int rc = do_search(v->quant, qb, qp, q_dtype, FX_MEM_DEVICE, np, (float*)v->coarse_d.p,
                                     (int64_t*)v->coarse_i.p, FX_MEM_DEVICE);
            if (rc != FX_OK) return rc;
        }
        if (v->profile) HIP_TRY(hipEventRecord(ev[1], s));
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
        ex.ex.D = Dd + q0 * k;
        ex.ex.I = Id + q0 * k;
        ex.d = v->d;
        ex.trained = v->tables;
        ex.cent = cent;
        if (!fused) {
            // the exact path for the whole pass: every query "flagged"
            HIP_TRY(launch_f32_queries(qp, q_dtype, qb, v->d, rb, (float*)v->qf32.p, s));
            HIP_TRY(launch_ivf_count_bad(ex.ex.coarse, qb * np, v->nlist, v->cnt + 2, s));
            HIP_TRY(launch_ivf_flag_all(n_flag, qb, s));
            if (v->profile) HIP_TRY(hipEventRecord(ev[2], s));
            HIP_TRY(launch_ivfsq_exact(v->metric, ex, s));
            if (v->profile) {  // (the exact scan is this path's "list scan"; it has no refine)
                HIP_TRY(hipEventRecord(ev[3], s));
                HIP_TRY(hipEventRecord(ev[4], s));
            }
            continue;
        }
        // 2. the pass's (query, list) pairs grouped by list, and their operands
        IvfPairs pr{};
        pr.coarse = ex.ex.coarse;
        pr.npairs = qb * np;
        pr.nlist = v->nlist;
        pr.list_off = v->list_off;
        pr.keys = (uint64_t*)v->pkeys.p;
        pr.sorted = (uint64_t*)v->psorted.p;
        pr.seg = (int*)v->seg.p;
        pr.ngrp = (int*)v->ngrp.p;
        pr.gbase = (int*)v->gbase.p;
        pr.bad = v->cnt + 2;
        HIP_TRY(launch_ivf_pairs(pr, v->ptemp.p, v->ptemp.bytes, s));
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
        sc.sorted = pr.sorted;
        sc.seg = pr.seg;
        sc.gbase = pr.gbase;
        sc.cand_d = (float*)v->cand_d.p;
        sc.cand_i = (int*)v->cand_i.p;
        sc.grid = (qb * np / TILE_Q + std::min<int64_t>(v->nlist, qb * np)) * C;
        if (v->profile) HIP_TRY(hipEventRecord(ev[2], s));
        HIP_TRY(launch_ivfsq_scan(v->metric, sc, s));
        if (v->profile) HIP_TRY(hipEventRecord(ev[3], s));
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
        if (v->profile) HIP_TRY(hipEventRecord(ev[4], s));
    }
    HIP_TRY(hipMemcpyAsync(v->pin_cnt, v->cnt, 12, hipMemcpyDeviceToHost, s));
    v->counts_pending = true;
    if (!host_out) return FX_OK;
    HIP_TRY(hipMemcpyAsync(D, Dd, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(I, Id, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s));
    if (const int rc = ivfsq_read_counts(v); rc != FX_OK) return rc;
    return v->last_dropped > 0 || v->last_bad_probe > 0 ? ivfsq_integrity(v) : FX_OK;
}

int fx_ivfsq_reset(FxIvfSq* v) {
    if (!v) return set_err(FX_E_ARG, "null ivfsq index");
    std::lock_guard<std::mutex> lk(v->mu);
    DeviceGuard g(v->device);
    hipStream_t s = v->stream();
    HIP_TRY(hipStreamSynchronize(s));
    // the maxima restart; the decode bound and the tables belong to the training and stay
    HIP_TRY(hipMemsetAsync(v->words, 0, 8, s));
    if (v->cap_rows > 0) {
        HIP_TRY(hipMemsetAsync(v->codes, 0, (size_t)v->cap_rows * v->row_bytes, s));
        HIP_TRY(hipMemsetAsync(v->nc, 0, (size_t)v->cap_rows * 4, s));
    }
    HIP_TRY(hipMemsetAsync(v->list_off, 0, (size_t)(v->nlist + 1) * 4, s));
    HIP_TRY(hipMemsetAsync(v->bad + 1, 0, 8, s));
    v->h_off.assign((size_t)v->nlist + 1, 0);
    v->ntotal = 0;
    v->max_list_rows = 0;
    v->dirty = false;
    v->sequential = false;
    v->counts_pending = false;
    v->last_fallbacks = v->last_dropped = v->last_bad_probe = 0;
    return FX_OK;
}

int fx_ivfsq_ntotal(const FxIvfSq* v, int64_t* out) {
    if (!v || !out) return set_err(FX_E_ARG, "null argument");
    *out = v->ntotal;
    return FX_OK;
}

int fx_ivfsq_list_sizes(FxIvfSq* v, int64_t* out) {
    if (!v || !out) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(v->mu);
    DeviceGuard g(v->device);
    if (const int rc = ivfsq_regroup(v); rc != FX_OK) return rc;
    for (int64_t l = 0; l < v->nlist; ++l) out[l] = (int64_t)v->h_off[l + 1] - v->h_off[l];
    return FX_OK;
}

int fx_ivfsq_list_ids(FxIvfSq* v, int64_t list, int64_t* out, int64_t cap, int64_t* n) {
    if (!v || !n) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(v->mu);
    if (list < 0 || list >= v->nlist)
        return set_err(FX_E_ARG, "ivfsq list_ids: list %lld outside [0, %lld)", (long long)list, (long long)v->nlist);
    DeviceGuard g(v->device);
    if (const int rc = ivfsq_regroup(v); rc != FX_OK) return rc;
    const int64_t r0 = v->h_off[list], cnt = (int64_t)v->h_off[list + 1] - r0;
    *n = cnt;
    if (cnt == 0 || cap <= 0) return FX_OK;
    if (!out) return set_err(FX_E_ARG, "null buffer");
    hipStream_t s = v->stream();
    HIP_TRY(hipMemcpyAsync(out, v->labels + r0, (size_t)std::min(cnt, cap) * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FX_OK;
}

int fx_ivfsq_list_codes(FxIvfSq* v, int64_t list, uint8_t* out, int64_t cap, int64_t* n) {
    if (!v || !n) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(v->mu);
    if (list < 0 || list >= v->nlist)
        return set_err(FX_E_ARG, "ivfsq list_codes: list %lld outside [0, %lld)", (long long)list, (long long)v->nlist);
    DeviceGuard g(v->device);
    if (const int rc = ivfsq_regroup(v); rc != FX_OK) return rc;
    const int64_t r0 = v->h_off[list], cnt = (int64_t)v->h_off[list + 1] - r0;
    *n = cnt;
    if (cnt == 0 || cap <= 0) return FX_OK;
    if (!out) return set_err(FX_E_ARG, "null buffer");
    const int64_t take = std::min(cnt, cap);
    hipStream_t s = v->stream();
    HIP_TRY(v->io.ensure((size_t)take * v->d));
    HIP_TRY(launch_ivfsq_codes_u8(v->codes, v->row_bytes, r0, take, v->d, (uint8_t*)v->io.p, s));
    HIP_TRY(hipMemcpyAsync(out, v->io.p, (size_t)take * v->d, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FX_OK;
}

int fx_ivfsq_set_stream(FxIvfSq* v, void* stream) {
    if (!v) return set_err(FX_E_ARG, "null ivfsq index");
    std::lock_guard<std::mutex> lk(v->mu);
    const hipStream_t prev = v->stream();
    v->user_stream = (hipStream_t)stream;
    const hipStream_t next = v->stream();
    if (next != prev) {
        DeviceGuard g(v->device);
        HIP_TRY(hipEventRecord(v->switch_ev, prev));
        HIP_TRY(hipStreamWaitEvent(next, v->switch_ev, 0));
    }
    return FX_OK;
}

int fx_ivfsq_last_counts(FxIvfSq* v, int64_t* fallbacks, int64_t* exact_fallbacks, int64_t* dropped) {
    if (!v || !fallbacks || !exact_fallbacks || !dropped) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(v->mu);
    if (const int rc = ivfsq_read_counts(v); rc != FX_OK) return rc;
    // (a flagged query goes straight to the exact list scan: both counts are the same)
    *fallbacks = v->last_fallbacks;
    *exact_fallbacks = v->last_fallbacks;
    *dropped = v->last_dropped + v->last_bad_probe;
    return FX_OK;
}

int fx_ivfsq_last_plan(FxIvfSq* v, int* path, int* chunks, int* slots, int64_t* q_batch, int64_t* grid) {
    if (!v || !path || !chunks || !slots || !q_batch || !grid) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(v->mu);
    *path = v->last_plan[0];
    *chunks = v->last_plan[1];
    *slots = v->last_plan[2];
    *q_batch = v->last_qbatch;
    *grid = v->last_grid;
    return FX_OK;
}

int fx_ivfsq_profile(FxIvfSq* v, int enable) {
    if (!v) return set_err(FX_E_ARG, "null ivfsq index");
    std::lock_guard<std::mutex> lk(v->mu);
    v->profile = enable != 0;
    return FX_OK;
}

int fx_ivfsq_profile_read(FxIvfSq* v, double* coarse_ms, double* pairs_ms, double* scan_ms, double* refine_ms,
                          int64_t* passes) {
    if (!v || !coarse_ms || !pairs_ms || !scan_ms || !refine_ms || !passes) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(v->mu);
    DeviceGuard g(v->device);
    HIP_TRY(hipStreamSynchronize(v->stream()));
    double ms[4] = {0, 0, 0, 0};
    float t = 0;
    for (size_t i = 0; i + 4 < v->ev.size(); i += 5)
        for (int part = 0; part < 4; ++part) {
            HIP_TRY(hipEventElapsedTime(&t, v->ev[i + part], v->ev[i + part + 1]));
            ms[part] += t;
        }
    *passes = (int64_t)(v->ev.size() / 5);
    for (hipEvent_t e : v->ev) (void)hipEventDestroy(e);
    v->ev.clear();
    *coarse_ms = ms[0];
    *pairs_ms = ms[1];
    *scan_ms = ms[2];
    *refine_ms = ms[3];
    return FX_OK;
}

}  // extern "C"

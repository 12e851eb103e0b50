// fx_api_kmeans.cpp -- k-means (fx_kmeans.hip): fx_kmeans_step / _update / _finish / _status.
#include "fx_host.h"

using namespace fx;

namespace {

// pinned staging of host training rows, per chunk
constexpr int64_t KMEANS_PIN_BYTES = 64ll << 20;

int km_check_index(const FxIndex* h, const char* who) {
    if (h->ntotal <= 0) return set_err(FX_E_ARG, "%s: the centroid index is empty", who);
    if (h->has_ids) return set_err(FX_E_UNSUPPORTED, "%s: the centroid index carries labels (add_with_ids)", who);
    if (h->id_offset != 0)
        return set_err(FX_E_UNSUPPORTED, "%s: the centroid index has id offset %lld", who, (long long)h->id_offset);
    if (h->ntotal > (int64_t)INT32_MAX) return set_err(FX_E_UNSUPPORTED, "%s: more than 2^31-1 centroids", who);
    return FX_OK;
}

hipError_t km_ensure_bad(FxIndex* h) {
    if (h->km.bad) return hipSuccess;
    hipError_t e = h->km.bad.ensure(8);
    if (e == hipSuccess) e = hipMemset(h->km.bad, 0, 8);
    if (e == hipSuccess) e = h->km.bad_pin.ensure(8);
    return e;
}

// the skipped-assignment count since the last read (waits for the stream), then 0 again
int km_read_bad(FxIndex* h, int64_t* out) {
    *out = 0;
    if (!h->km.bad) return FX_OK;
    hipStream_t s = h->stream();
    HIP_TRY(hipMemcpyAsync(h->km.bad_pin, h->km.bad, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemsetAsync(h->km.bad, 0, 8, s));
    HIP_TRY(hipStreamSynchronize(s));
    *out = (int64_t)*h->km.bad_pin;
    return FX_OK;
}

int km_bad_error(int64_t bad, int64_t k) {
    return set_err(FX_E_INTEGRITY, "kmeans: %lld assignments outside [0, %lld) were skipped", (long long)bad,
                   (long long)k);
}

// fx_kmeans_step (search) / fx_kmeans_update: the rows in chunks, each chunk's
// assignment (searched, or the caller's) and its update, accumulated in chunk order
int km_run(FxIndex* h, int64_t n, const void* x, int x_dtype, int x_mem, int64_t* assign, float* dist, bool search,
           double* sums, int64_t* counts, double* obj, int accumulate) {
    hipStream_t s = h->stream();
    const int64_t k = h->ntotal;
    const int64_t rowb = (int64_t)h->d * dtype_size(x_dtype);
    const bool host = x_mem == FX_MEM_HOST;
    int64_t chunk = h->opt.kmeans_chunk > 0 ? h->opt.kmeans_chunk : (int)KMEANS_CHUNK_DEFAULT;
    if (host) chunk = std::min(chunk, std::max<int64_t>(1, KMEANS_PIN_BYTES / rowb));
    chunk = std::min(chunk, n);
    HIP_TRY(km_ensure_bad(h));
    if (search && (!assign || !dist)) HIP_TRY(h->km.out.ensure((size_t)chunk * 12));
    if (host) {
        HIP_TRY(h->km.x.ensure((size_t)(chunk * rowb)));
        HIP_TRY(h->km.pin.ensure((size_t)(chunk * rowb)));
    }
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t nr = std::min(chunk, n - r0);
        size_t ws_bytes = 0;  // (per chunk: the sort's temporaries need not grow with the rows)
        HIP_TRY(km_workspace(nr, k, h->d, &ws_bytes));
        HIP_TRY(h->km.ws.ensure(ws_bytes));
        const void* xd = (const char*)x + r0 * rowb;
        if (host) {
            memcpy(h->km.pin.p, xd, (size_t)(nr * rowb));
            HIP_TRY(hipMemcpyAsync(h->km.x.p, h->km.pin.p, (size_t)(nr * rowb), hipMemcpyHostToDevice, s));
            xd = h->km.x.p;
        }
        int64_t* a = assign ? assign + r0 : (int64_t*)h->km.out.p;
        float* dd = dist ? dist + r0 : (search ? (float*)((char*)h->km.out.p + (size_t)chunk * 8) : nullptr);
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        if (h->profile) {
            for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
            h->km.ev.insert(h->km.ev.end(), ev, ev + 4);
            HIP_TRY(hipEventRecord(ev[0], s));
        }
        if (search) {
            // the index's own device-output k = 1 search: every plan, the re-scan and the exact fallback
            const int rc = do_search(h, nr, xd, x_dtype, FX_MEM_DEVICE, 1, dd, a, FX_MEM_DEVICE);
            if (rc != FX_OK) return rc;
        }
        if (h->profile) HIP_TRY(hipEventRecord(ev[1], s));
        KmUpdate u{};
        u.x = xd;
        u.x_dt = x_dtype;
        u.n = nr;
        u.d = h->d;
        u.k = k;
        u.assign = a;
        u.dist = dd;
        u.sums = sums;
        u.counts = counts;
        u.obj = obj;
        u.accumulate = accumulate != 0 || r0 > 0;
        u.bad = h->km.bad;
        HIP_TRY(launch_km_update(u, h->km.ws.p, h->km.ws.bytes, s, ev[2]));
        if (h->profile) HIP_TRY(hipEventRecord(ev[3], s));
        if (host) HIP_TRY(hipStreamSynchronize(s));  // (the staging buffers are free again)
    }
    if (!host) return FX_OK;
    // a host call has waited for its work: its skipped entries are known now
    int64_t bad = 0;
    if (const int rc = km_read_bad(h, &bad); rc != FX_OK) return rc;
    return bad > 0 ? km_bad_error(bad, k) : FX_OK;
}

int km_check_args(const FxIndex* h, int64_t n, int x_dtype, int x_mem, const double* sums, const int64_t* counts,
                  const double* obj) {
    // (the index last: the other checks are then reachable without a device)
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (!check_dtype(x_dtype)) return set_err(FX_E_ARG, "bad x dtype %d", x_dtype);
    if (!valid_mem(x_mem)) return set_err(FX_E_ARG, "bad x_mem %d", x_mem);
    if (!sums || !counts || !obj) return set_err(FX_E_ARG, "null sums / counts / obj");
    if (!h) return set_err(FX_E_ARG, "null index");
    return FX_OK;
}

}  // namespace

extern "C" {

int fx_kmeans_step(FxIndex* h, int64_t n, const void* x, int x_dtype, int x_mem, int64_t* assign, float* dist,
                   double* sums, int64_t* counts, double* obj, int accumulate) {
    if (const int rc = km_check_args(h, n, x_dtype, x_mem, sums, counts, obj); rc != FX_OK) return rc;
    if (n == 0) return FX_OK;
    if (!x) return set_err(FX_E_ARG, "null x");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = km_check_index(h, "kmeans_step"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    return km_run(h, n, x, x_dtype, x_mem, assign, dist, true, sums, counts, obj, accumulate);
}

int fx_kmeans_update(FxIndex* h, int64_t n, const void* x, int x_dtype, int x_mem, const int64_t* assign,
                     const float* dist, double* sums, int64_t* counts, double* obj, int accumulate) {
    if (const int rc = km_check_args(h, n, x_dtype, x_mem, sums, counts, obj); rc != FX_OK) return rc;
    if (n == 0) return FX_OK;
    if (!x || !assign) return set_err(FX_E_ARG, "null x / assign");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = km_check_index(h, "kmeans_update"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    return km_run(h, n, x, x_dtype, x_mem, const_cast<int64_t*>(assign), const_cast<float*>(dist), false, sums, counts,
                  obj, accumulate);
}

int fx_kmeans_finish(FxIndex* h, const double* sums, const int64_t* counts, int spherical, float* centroids_out,
                     int64_t* n_split) {
    if (!sums || !counts || !centroids_out || !n_split) return set_err(FX_E_ARG, "null buffer");
    if (!h) return set_err(FX_E_ARG, "null index");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = km_check_index(h, "kmeans_finish"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    hipStream_t s = h->stream();
    const int64_t k = h->ntotal;
    HIP_TRY(h->km.h.ensure((size_t)k * 8));
    hipEvent_t ev[2] = {nullptr, nullptr};
    if (h->profile) {
        for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
        h->km.ev_fin.insert(h->km.ev_fin.end(), ev, ev + 2);
        HIP_TRY(hipEventRecord(ev[0], s));
    }
    KmFinish f{};
    f.sums = sums;
    f.counts = counts;
    f.k = k;
    f.d = h->d;
    f.codes = h->codes;
    f.st_dt = h->dtype;
    f.row_bytes = h->row_bytes;
    f.spherical = spherical;
    f.cent = centroids_out;
    f.h = (int64_t*)h->km.h.p;
    f.n_split = n_split;
    HIP_TRY(launch_km_finish(f, s));
    // fx_index_reset and a device-side fx_index_add of the k new rows, both
    // stream-ordered: the rows [0, k) are rewritten in place (nothing grows, the
    // rows past k keep their zero codes and +inf norms), the scan image and
    // its centre are rebuilt by the next search, selectors from before are stale
    HIP_TRY(hipMemsetAsync(h->max_sq_bits, 0, 8, s));
    h->ntotal = 0;
    ++h->epoch;
    h->img_rows = 0;
    h->mu_rows = 0;
    h->rg.nq = -1;
    h->rg.total = 0;
    if (const int rc = append_rows(h, k, centroids_out, FX_F32, FX_MEM_DEVICE); rc != FX_OK) return rc;
    h->ntotal = k;
    if (h->profile) HIP_TRY(hipEventRecord(ev[1], s));
    return FX_OK;
}

int fx_kmeans_status(FxIndex* h, int64_t* bad_assign) {
    if (!h || !bad_assign) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    if (const int rc = km_read_bad(h, bad_assign); rc != FX_OK) return rc;
    return *bad_assign > 0 ? km_bad_error(*bad_assign, h->ntotal) : FX_OK;
}

int fx_kmeans_profile_read(FxIndex* h, double* assign_ms, double* sort_ms, double* sum_ms, double* finish_ms) {
    if (!h || !assign_ms || !sort_ms || !sum_ms || !finish_ms) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream()));
    double ms[4] = {0, 0, 0, 0};
    float v = 0;
    for (size_t i = 0; i + 3 < h->km.ev.size(); i += 4)
        for (int p = 0; p < 3; ++p) {
            HIP_TRY(hipEventElapsedTime(&v, h->km.ev[i + p], h->km.ev[i + p + 1]));
            ms[p] += v;
        }
    for (size_t i = 0; i + 1 < h->km.ev_fin.size(); i += 2) {
        HIP_TRY(hipEventElapsedTime(&v, h->km.ev_fin[i], h->km.ev_fin[i + 1]));
        ms[3] += v;
    }
    for (hipEvent_t e : h->km.ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->km.ev_fin) (void)hipEventDestroy(e);
    h->km.ev.clear();
    h->km.ev_fin.clear();
    *assign_ms = ms[0];
    *sort_ms = ms[1];
    *sum_ms = ms[2];
    *finish_ms = ms[3];
    return FX_OK;
}

}  // extern "C"

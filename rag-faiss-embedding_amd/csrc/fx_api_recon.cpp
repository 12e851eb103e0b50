// fx_api_recon.cpp -- stored vectors and distances by key (fx_recon.hip): reconstruct_n / _batch,
// search_and_reconstruct, compute_distance_subset.
#include "fx_host.h"

using namespace fx;

namespace {

// bytes of the bounded stage buffer a host read-back goes through per chunk
constexpr int64_t RECON_STAGE_BYTES = 128ll << 20;

// Rows by key -> host `out`, in chunks through the stage buffer (one gather,
// one device-to-host copy and one wait per chunk).  keys: n int64 on the
// device, or null for the implicit keys key0 + i.
int gather_to_host(FxIndex* h, const int64_t* keys, int64_t key0, int64_t id_offset, int64_t n, void* out,
                   int out_dtype) {
    hipStream_t s = h->stream();
    const int64_t rowb = (int64_t)h->d * dtype_size(out_dtype);
    const int64_t chunk = std::max<int64_t>(1, RECON_STAGE_BYTES / rowb);
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t nr = std::min(chunk, n - r0);
        HIP_TRY(h->stage.ensure((size_t)(nr * rowb)));
        HIP_TRY(launch_gather_rows(h->codes, h->dtype, h->row_bytes, h->ntotal, keys ? keys + r0 : nullptr, key0 + r0,
                                   id_offset, nr, h->d, h->stage.p, out_dtype, s));
        HIP_TRY(hipMemcpyAsync((char*)out + (size_t)(r0 * rowb), h->stage.p, (size_t)(nr * rowb), hipMemcpyDeviceToHost,
                               s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return FX_OK;
}

// the keys of a labelled index (n <= INT_MAX labels on the device) as rows in
// h->rc.rows: the last row of a label, -1 when none; one pass over the labels
int rows_of_keys(FxIndex* h, const int64_t* dkeys, int64_t n, const int64_t** rows) {
    size_t sort_bytes = 0;
    HIP_TRY(idmap_sort_bytes(n, true, &sort_bytes));
    HIP_TRY(h->idm.ws.ensure(sort_bytes));
    HIP_TRY(h->rc.rows.ensure((size_t)n * 8));
    HIP_TRY(launch_rows_of_labels(h->idm.labels, h->ntotal, dkeys, n, (int64_t*)h->rc.rows.p, h->idm.ws.p, sort_bytes,
                                  h->stream()));
    *rows = (const int64_t*)h->rc.rows.p;
    return FX_OK;
}

}  // namespace

extern "C" {

int fx_index_reconstruct_n(FxIndex* h, int64_t i0, int64_t n, float* out) {
    if (!h || !out || i0 < 0 || n < 0) return set_err(FX_E_ARG, "bad reconstruct range");
    std::lock_guard<std::mutex> lk(h->mu);
    if (i0 > h->ntotal || n > h->ntotal - i0) return set_err(FX_E_ARG, "bad reconstruct range");
    if (n == 0) return FX_OK;
    DeviceGuard g(h->device);
    // the implicit keys i0 + i of rows [i0, i0 + n)
    return gather_to_host(h, nullptr, i0, 0, n, out, FX_F32);
}

int fx_index_reconstruct_batch(FxIndex* h, int64_t n, const int64_t* keys, int keys_mem, void* out, int out_dtype,
                               int out_mem) {
    if (!check_dtype(out_dtype))
        return set_err(FX_E_UNSUPPORTED, "reconstruct_batch: out_dtype %d is neither FX_F32 nor a storage dtype", out_dtype);
    if (!h) return set_err(FX_E_ARG, "null index");
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (!valid_mem(keys_mem) || !valid_mem(out_mem))
        return set_err(FX_E_ARG, "bad keys_mem / out_mem");
    if (n > (int64_t)INT32_MAX) return set_err(FX_E_UNSUPPORTED, "reconstruct_batch: more than 2^31-1 keys per call");
    std::lock_guard<std::mutex> lk(h->mu);
    if (out_dtype != FX_F32 && out_dtype != h->dtype)
        return set_err(FX_E_UNSUPPORTED, "reconstruct_batch: out_dtype %d is neither FX_F32 nor the index's storage dtype %d",
                       out_dtype, h->dtype);
    if (n == 0) return FX_OK;
    if (!keys || !out) return set_err(FX_E_ARG, "null buffer");
    // host keys of an unlabelled index are checked here, before anything is written (faiss asserts
    // key < ntotal); device keys cannot be without a sync: a bad one yields a NaN row
    if (keys_mem == FX_MEM_HOST && !h->has_ids)
        for (int64_t i = 0; i < n; ++i)
            if (keys[i] < h->id_offset || keys[i] - h->id_offset >= h->ntotal)
                return set_err(FX_E_ARG, "reconstruct_batch: key %lld (entry %lld) outside the index's ids [%lld, %lld)",
                               (long long)keys[i], (long long)i, (long long)h->id_offset,
                               (long long)(h->id_offset + h->ntotal));
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    hipStream_t s = h->stream();
    const void* staged = nullptr;
    HIP_TRY(stage_in(h->stream(), h->rc.in, keys, (size_t)n * 8, keys_mem, &staged));
    const int64_t* dkeys = (const int64_t*)staged;
    int64_t id_offset = h->id_offset;
    if (h->has_ids) {  // labels -> rows (an unknown label: -1 -> a NaN row)
        const int rc = rows_of_keys(h, dkeys, n, &dkeys);
        if (rc != FX_OK) return rc;
        id_offset = 0;
    }
    if (out_mem == FX_MEM_HOST) return gather_to_host(h, dkeys, 0, id_offset, n, out, out_dtype);
    HIP_TRY(launch_gather_rows(h->codes, h->dtype, h->row_bytes, h->ntotal, dkeys, 0, id_offset, n, h->d, out,
                               out_dtype, s));
    // (host keys: the call is done with the caller's array when it returns)
    if (keys_mem == FX_MEM_HOST) HIP_TRY(hipStreamSynchronize(s));
    return FX_OK;
}

int fx_index_search_and_reconstruct(FxIndex* h, const FxSelector* sel, int64_t nq, const void* q, int q_dtype,
                                    int q_mem, int k, float* D, int64_t* I, void* R, int r_dtype, int out_mem) {
    if (!h) return set_err(FX_E_ARG, "null index");
    if (nq < 0) return set_err(FX_E_ARG, "negative nq");
    if (k <= 0) return set_err(FX_E_ARG, "k must be positive (got %d)", k);
    if (!check_dtype(q_dtype)) return set_err(FX_E_ARG, "bad query dtype %d", q_dtype);
    if (!valid_mem(q_mem) || !valid_mem(out_mem))
        return set_err(FX_E_ARG, "bad q_mem / out_mem");
    if (!check_dtype(r_dtype))
        return set_err(FX_E_UNSUPPORTED, "search_and_reconstruct: r_dtype %d is neither FX_F32 nor a storage dtype", r_dtype);
    if (sel)
        if (const int rc = check_selector(h, sel, "search", nullptr); rc != FX_OK) return rc;
    if (sel && k > FX_MAX_K)
        return set_err(FX_E_UNSUPPORTED, "search with a selector supports k <= %d (got %d): the exact sort path takes none",
                       FX_MAX_K, k);
    if (nq == 0) return FX_OK;
    if (!q || !D || !I || !R) return set_err(FX_E_ARG, "null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (r_dtype != FX_F32 && r_dtype != h->dtype)
        return set_err(FX_E_UNSUPPORTED, "search_and_reconstruct: r_dtype %d is neither FX_F32 nor the index's storage "
                       "dtype %d", r_dtype, h->dtype);
    if (sel)
        if (const int rc = check_selector(h, sel, "search", "rows were added or the index was reset"); rc != FX_OK)
            return rc;
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    if (sel) {
        const int rc = selector_counts(sel);
        if (rc != FX_OK) return rc;
    }
    hipStream_t s = h->stream();
    const bool host_out = out_mem == FX_MEM_HOST;
    const size_t nres = (size_t)nq * k, rbytes = nres * h->d * dtype_size(r_dtype);
    // nothing to rank: every slot missing, every vector NaN
    if (h->ntotal == 0 || (sel && sel->rows == 0)) {
        const int rc = fill_missing(h, nq, k, D, I, out_mem);
        if (rc != FX_OK) return rc;
        if (host_out) memset(R, 0xff, rbytes);
        else HIP_TRY(hipMemsetAsync(R, 0xff, rbytes, s));
        return FX_OK;
    }
    // The search itself, device-resident and eager (never a search graph), reporting ROWS (+ id_offset)
    // also on a labelled index: the gather must read the row that ranked, and labels may repeat.
    float* Dd = D;
    int64_t* Id = I;
    const size_t offI = (size_t)round_up((int64_t)nres * 4, 256);
    if (host_out) {
        HIP_TRY(h->rc.out.ensure(offI + nres * 8));
        Dd = (float*)h->rc.out.p;
        Id = (int64_t*)((char*)h->rc.out.p + offI);
    }
    const int rc = !sel && k > FX_MAX_K
                       ? do_search_hugek(h, nq, q, q_dtype, q_mem, k, Dd, Id, FX_MEM_DEVICE, true)
                       : do_search(h, nq, q, q_dtype, q_mem, k, Dd, Id, FX_MEM_DEVICE, sel, true);
    if (rc != FX_OK) return rc;
    // the gather follows the re-scan / exact-fallback chain on the stream; a missing slot's -1 is no row: NaN
    if (host_out) {
        const int rg = gather_to_host(h, Id, 0, h->id_offset, (int64_t)nres, R, r_dtype);
        if (rg != FX_OK) return rg;
    } else {
        HIP_TRY(launch_gather_rows(h->codes, h->dtype, h->row_bytes, h->ntotal, Id, 0, h->id_offset, (int64_t)nres,
                                   h->d, R, r_dtype, s));
    }
    if (h->has_ids) HIP_TRY(launch_label_ids(h->idm.labels, h->ntotal, (int64_t)nres, Id, s));
    if (host_out) {
        HIP_TRY(hipMemcpyAsync(D, Dd, nres * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(I, Id, nres * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return read_counts(h);  // (a host result checks the candidate lists' integrity itself, as search does)
    } else if (q_mem == FX_MEM_HOST) {
        HIP_TRY(hipStreamSynchronize(s));  // (host queries: done with the caller's array on return)
    }
    return FX_OK;
}

int fx_index_compute_distance_subset(FxIndex* h, int64_t nq, const void* q, int q_dtype, int q_mem, int k,
                                     const int64_t* keys, int keys_mem, float* D, int out_mem) {
    if (!h) return set_err(FX_E_ARG, "null index");
    if (nq < 0) return set_err(FX_E_ARG, "negative nq");
    if (k <= 0) return set_err(FX_E_ARG, "k must be positive (got %d)", k);
    if (!check_dtype(q_dtype)) return set_err(FX_E_ARG, "bad query dtype %d", q_dtype);
    if (!valid_mem(q_mem) || !valid_mem(keys_mem) ||
        !valid_mem(out_mem))
        return set_err(FX_E_ARG, "bad q_mem / keys_mem / out_mem");
    if (nq == 0) return FX_OK;
    if (!q || !keys || !D) return set_err(FX_E_ARG, "null buffer");
    if (nq > (int64_t)INT32_MAX / k)
        return set_err(FX_E_UNSUPPORTED, "compute_distance_subset: more than 2^31-1 (query, key) pairs per call");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    hipStream_t s = h->stream();
    const int64_t n = nq * k;
    // host inputs staged in one buffer: [queries | keys]
    const size_t qbytes = (size_t)nq * h->d * dtype_size(q_dtype), koff = (size_t)round_up((int64_t)qbytes, 256);
    const bool stage_q = q_mem == FX_MEM_HOST, stage_k = keys_mem == FX_MEM_HOST;
    if (stage_q || stage_k) HIP_TRY(h->rc.in.ensure(koff + (size_t)n * 8));
    const void *qdev = nullptr, *staged = nullptr;
    HIP_TRY(stage_in(h->stream(), h->rc.in, q, qbytes, q_mem, &qdev));
    HIP_TRY(stage_in(h->stream(), h->rc.in, keys, (size_t)n * 8, keys_mem, &staged, koff));
    const int64_t* dkeys = (const int64_t*)staged;
    // the queries once as padded fp32 [nq][kdim], in a buffer of this call's own (not a search's)
    HIP_TRY(h->rc.qf32.ensure((size_t)nq * h->kdim * 4));
    HIP_TRY(launch_f32_queries(qdev, q_dtype, nq, h->d, h->kdim, (float*)h->rc.qf32.p, s));
    int64_t id_offset = h->id_offset;
    if (h->has_ids) {
        const int rc = rows_of_keys(h, dkeys, n, &dkeys);
        if (rc != FX_OK) return rc;
        id_offset = 0;
    }
    float* Dd = D;
    if (out_mem == FX_MEM_HOST) {
        HIP_TRY(h->rc.out.ensure((size_t)n * 4));
        Dd = (float*)h->rc.out.p;
    }
    HIP_TRY(launch_subset_dist(h->dtype, h->metric, h->codes, h->row_bytes, h->kdim, h->ntotal,
                               (const float*)h->rc.qf32.p, nq, k, dkeys, id_offset, Dd, s));
    if (out_mem == FX_MEM_HOST) HIP_TRY(hipMemcpyAsync(D, Dd, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (out_mem == FX_MEM_HOST || stage_q || stage_k) HIP_TRY(hipStreamSynchronize(s));
    return FX_OK;
}

}  // extern "C"

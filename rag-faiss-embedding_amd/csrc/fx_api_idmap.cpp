// fx_api_idmap.cpp -- stable ids (fx_idmap.hip): add_with_ids, get_ids, rows_of_ids.
#include "fx_host.h"

using namespace fx;

extern "C" {

int fx_index_add_with_ids(FxIndex* h, int64_t n, const void* x, int x_dtype, int x_mem, const int64_t* ids,
                          int ids_mem) {
    if (!h) return set_err(FX_E_ARG, "null index");
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (n == 0) return FX_OK;
    if (!ids) return set_err(FX_E_ARG, "add_with_ids: null ids");
    if (!valid_mem(ids_mem)) return set_err(FX_E_ARG, "bad ids_mem %d", ids_mem);
    if (const int rc = check_add_args(h, n, x, x_dtype); rc != FX_OK) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->has_ids && h->ntotal > 0)
        return set_err(FX_E_ARG, "add_with_ids not implemented for an index that holds rows without labels");
    if (h->id_offset != 0)
        return set_err(FX_E_ARG, "add_with_ids: the index has id offset %lld; labels and an id offset exclude each other",
                       (long long)h->id_offset);
    DeviceGuard g(h->device);
    const bool was = h->has_ids;
    h->has_ids = true;  // (grow carries / allocates the label buffer from here on)
    int rc = append_rows(h, n, x, x_dtype, x_mem);
    if (rc == FX_OK) {
        hipStream_t s = h->stream();
        hipError_t e = hipMemcpyAsync(h->idm.labels + h->ntotal, ids, (size_t)n * 8,
                                      ids_mem == FX_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s);
        // (host ids: the caller's array may go when the call returns)
        if (e == hipSuccess && ids_mem == FX_MEM_HOST) e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = set_err(FX_E_HIP, "add_with_ids: copying the labels: %s", hipGetErrorString(e));
    }
    if (rc != FX_OK) {
        h->has_ids = was;
        return rc;
    }
    h->ntotal += n;
    return FX_OK;
}

int fx_index_has_ids(const FxIndex* h, int* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    *out = h->has_ids ? 1 : 0;
    return FX_OK;
}

int fx_index_get_ids(FxIndex* h, int64_t i0, int64_t n, int64_t* out, int out_mem) {
    if (!h) return set_err(FX_E_ARG, "null index");
    if (i0 < 0 || n < 0) return set_err(FX_E_ARG, "get_ids: negative range");
    if (!valid_mem(out_mem)) return set_err(FX_E_ARG, "bad out_mem %d", out_mem);
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->has_ids) return set_err(FX_E_ARG, "get_ids: the index carries no labels (it was not filled by add_with_ids)");
    if (i0 > h->ntotal || n > h->ntotal - i0)
        return set_err(FX_E_ARG, "get_ids: rows [%lld, %lld) outside the index's %lld", (long long)i0,
                       (long long)(i0 + n), (long long)h->ntotal);
    if (n == 0) return FX_OK;
    if (!out) return set_err(FX_E_ARG, "null buffer");
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    HIP_TRY(hipMemcpyAsync(out, h->idm.labels + i0, (size_t)n * 8,
                           out_mem == FX_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
    if (out_mem == FX_MEM_HOST) HIP_TRY(hipStreamSynchronize(s));
    return FX_OK;
}

int fx_index_rows_of_ids(FxIndex* h, const int64_t* ids, int64_t n, int ids_mem, int64_t* rows, int rows_mem) {
    if (!h) return set_err(FX_E_ARG, "null index");
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (!valid_mem(ids_mem) || !valid_mem(rows_mem))
        return set_err(FX_E_ARG, "bad ids_mem / rows_mem");
    if (n > 0 && (!ids || !rows)) return set_err(FX_E_ARG, "null buffer");
    if (n > (int64_t)INT32_MAX) return set_err(FX_E_UNSUPPORTED, "rows_of_ids: more than 2^31-1 ids per call");
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->has_ids) return set_err(FX_E_ARG, "rows_of_ids: the index carries no labels (it was not filled by add_with_ids)");
    if (n == 0) return FX_OK;
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    // workspace: [sort | staged host ids | device rows of a host output]
    size_t sort_bytes = 0;
    HIP_TRY(idmap_sort_bytes(n, true, &sort_bytes));
    const size_t nb = (size_t)round_up(n * 8, 256);
    HIP_TRY(h->idm.ws.ensure(sort_bytes + 2 * nb));
    char* base = (char*)h->idm.ws.p;
    const void* dids = nullptr;
    HIP_TRY(stage_in(h->stream(), h->idm.ws, ids, (size_t)n * 8, ids_mem, &dids, sort_bytes));
    int64_t* drows = rows_mem == FX_MEM_HOST ? (int64_t*)(base + sort_bytes + nb) : rows;
    HIP_TRY(launch_rows_of_labels(h->idm.labels, h->ntotal, (const int64_t*)dids, n, drows, base, sort_bytes, s));
    if (rows_mem == FX_MEM_HOST) HIP_TRY(hipMemcpyAsync(rows, drows, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    // (host buffers on either side: the call is done with them when it returns)
    if (rows_mem == FX_MEM_HOST || ids_mem == FX_MEM_HOST) HIP_TRY(hipStreamSynchronize(s));
    return FX_OK;
}

}  // extern "C"

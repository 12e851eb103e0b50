// fx_api_select.cpp -- filtered search (fx_select.hip): selectors and fx_index_search_sel.
#include "fx_host.h"

using namespace fx;

// the selector's counts on the host (waits for its build once)
int fx::selector_counts(const FxSelector* sel) {
    std::lock_guard<std::mutex> lk(sel->mu);
    if (sel->known) return FX_OK;
    DeviceGuard g(sel->device);
    HIP_TRY(hipEventSynchronize(sel->ready));
    sel->rows = sel->pin[0].rows;
    sel->ntiles = sel->pin[0].tiles;
    sel->known = true;
    return FX_OK;
}

int fx::check_selector(const FxIndex* h, const FxSelector* sel, const char* who, const char* since) {
    if (sel->index != h) return set_err(FX_E_ARG, "%s: the selector was created on another index", who);
    if (since && (sel->ntotal != h->ntotal || sel->epoch != h->epoch))
        return set_err(FX_E_ARG, "%s: stale selector: it is a snapshot of %lld rows, the index now has %lld "
                       "(%s since it was created)", who, (long long)sel->ntotal, (long long)h->ntotal, since);
    return FX_OK;
}

extern "C" {

void fx_selector_free(FxSelector* sel) {
    if (!sel) return;
    DeviceGuard g(sel->device);
    if (sel->ready) {
        (void)hipEventSynchronize(sel->ready);
        (void)hipEventDestroy(sel->ready);
    }
    delete sel;  // (its buffers free themselves, with the selector's device current)
}

int fx_selector_create(FxIndex* h, int kind, const void* data, int64_t n, int data_mem, int invert,
                       FxSelector** out) {
    if (!out) return set_err(FX_E_ARG, "null out");
    *out = nullptr;
    if (kind != FX_SEL_BITMAP && kind != FX_SEL_IDS && kind != FX_SEL_RANGE)
        return set_err(FX_E_ARG, "bad selector kind %d (FX_SEL_BITMAP 0, FX_SEL_IDS 1, FX_SEL_RANGE 2)", kind);
    if (!h) return set_err(FX_E_ARG, "null index");
    if (!valid_mem(data_mem)) return set_err(FX_E_ARG, "bad data_mem %d", data_mem);
    int64_t imin = 0, imax = 0;
    if (kind == FX_SEL_RANGE) {
        if (!data) return set_err(FX_E_ARG, "selector: null range");
        memcpy(&imin, data, 8);
        memcpy(&imax, (const char*)data + 8, 8);
        if (imax < imin)
            return set_err(FX_E_ARG, "selector: range with imax %lld < imin %lld", (long long)imax, (long long)imin);
    } else {
        if (n < 0) return set_err(FX_E_ARG, "selector: negative n");
        if (n > 0 && !data) return set_err(FX_E_ARG, "selector: null data");
    }
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    hipStream_t s = h->stream();
    FxSelector* sel = new FxSelector();
    sel->index = h;
    sel->device = h->device;
    sel->ntotal = h->ntotal;
    sel->epoch = h->epoch;
    const int64_t nt = h->ntotal, off = h->id_offset;
    const int64_t nwords = sel_mask_words(nt), ntiles = nwords / (TILE_R / 32);
    DevBuf staged;  // host data on the device for the build (an unlabelled index)
    hipError_t e = sel->mask.ensure((size_t)std::max<int64_t>(nwords, 4) * 4);
    if (e == hipSuccess) e = sel->tiles.ensure((size_t)std::max<int64_t>(ntiles, 1) * 4);
    if (e == hipSuccess) e = sel->cnt.ensure(sizeof(SelCounts));
    if (e == hipSuccess) e = sel->pin.ensure(sizeof(SelCounts));
    if (e == hipSuccess) e = hipEventCreateWithFlags(&sel->ready, hipEventDisableTiming);
    // a labelled index (fx_idmap.hip): ids, range bounds and bitmap bits mean labels
    const int64_t* labels = h->label_ptr();
    if (e == hipSuccess && labels && nt > 0) {
        if (kind == FX_SEL_RANGE) {
            e = launch_sel_range_lbl(labels, imin, imax, nt, invert != 0, sel->mask, s);
        } else {
            const size_t bytes = (size_t)n * (kind == FX_SEL_IDS ? 8 : 1);
            // index-owned scratch: [sort workspace of the id list | host data staged for the build]
            size_t sort_bytes = 0;
            if (kind == FX_SEL_IDS && n > 0) {
                if (n > (int64_t)INT32_MAX) e = hipErrorInvalidValue;
                else e = idmap_sort_bytes(n, false, &sort_bytes);
            }
            const bool stage = data_mem == FX_MEM_HOST && n > 0;
            if (e == hipSuccess && sort_bytes + (stage ? bytes : 0) > 0)
                e = h->idm.ws.ensure(sort_bytes + (stage ? bytes : 0));
            const void* dev = data;
            if (e == hipSuccess && stage) e = stage_in(h->stream(), h->idm.ws, data, bytes, data_mem, &dev, sort_bytes);
            if (e == hipSuccess)
                e = kind == FX_SEL_IDS
                        ? launch_sel_ids_lbl(labels, (const int64_t*)dev, n, nt, invert != 0, sel->mask, h->idm.ws.p,
                                             sort_bytes, s)
                        : launch_sel_bitmap_lbl(labels, (const uint8_t*)dev, n, nt, invert != 0, sel->mask, s);
            // (host data: the pageable copy above has to be out of the caller's array before the call returns)
            if (e == hipSuccess && stage) e = hipStreamSynchronize(s);
        }
    } else if (e == hipSuccess && kind == FX_SEL_RANGE) {
        // ids -> local rows, clamped to the index (id_offset >= 0; differences of int64 ids may not overflow)
        auto local = [&](int64_t id) { return id <= off ? (int64_t)0 : std::min(id - off, nt); };
        e = launch_sel_range(local(imin), local(imax), nt, invert != 0, sel->mask, s);
    } else if (e == hipSuccess) {
        const size_t bytes = (size_t)n * (kind == FX_SEL_IDS ? 8 : 1);
        const void* dev = data;
        if (n > 0) e = stage_in(h->stream(), staged, data, bytes, data_mem, &dev);
        if (e == hipSuccess)
            e = kind == FX_SEL_IDS ? launch_sel_ids((const int64_t*)dev, n, off, nt, invert != 0, sel->mask, s)
                                   : launch_sel_bitmap((const uint8_t*)dev, n, off, nt, invert != 0, sel->mask, s);
    }
    if (e == hipSuccess) e = launch_sel_tiles(sel->mask, nt, sel->tiles, sel->cnt, s);
    if (e == hipSuccess) e = hipMemcpyAsync(sel->pin, sel->cnt, sizeof(SelCounts), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipEventRecord(sel->ready, s);
    // host data: the build has to finish before the staging copy goes (on return)
    if (staged.p && e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        fx_selector_free(sel);
        return set_err(FX_E_HIP, "selector build: %s", hipGetErrorString(e));
    }
    *out = sel;
    return FX_OK;
}

int fx_selector_stats(const FxSelector* sel, int64_t* rows, int64_t* tiles) {
    if (!sel || !rows || !tiles) return set_err(FX_E_ARG, "null argument");
    const int rc = selector_counts(sel);
    if (rc != FX_OK) return rc;
    *rows = sel->rows;
    *tiles = sel->ntiles;
    return FX_OK;
}

int fx_index_search_sel(FxIndex* h, const FxSelector* sel, int64_t nq, const void* q, int q_dtype, int q_mem, int k,
                        float* D, int64_t* I, int out_mem) {
    if (!h) return set_err(FX_E_ARG, "null index");
    if (!sel) return set_err(FX_E_ARG, "null selector");
    if (nq < 0) return set_err(FX_E_ARG, "negative nq");
    if (k <= 0) return set_err(FX_E_ARG, "k must be positive (got %d)", k);
    if (!check_dtype(q_dtype)) return set_err(FX_E_ARG, "bad query dtype %d", q_dtype);
    if (const int rc = check_selector(h, sel, "search", nullptr); rc != FX_OK) return rc;
    if (k > FX_MAX_K)
        return set_err(FX_E_UNSUPPORTED, "search with a selector supports k <= %d (got %d): the exact sort path takes none",
                       FX_MAX_K, k);
    if (nq == 0) return FX_OK;
    if (!q || !D || !I) return set_err(FX_E_ARG, "null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = check_selector(h, sel, "search", "rows were added or the index was reset"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    {
        const int rc = selector_counts(sel);
        if (rc != FX_OK) return rc;
    }
    // nothing selected (or an empty index): every slot missing, no scan
    if (h->ntotal == 0 || sel->rows == 0) return fill_missing(h, nq, k, D, I, out_mem);
    return do_search(h, nq, q, q_dtype, q_mem, k, D, I, out_mem, sel);
}

}  // extern "C"

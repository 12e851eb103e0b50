// fx_index.cpp -- host implementation of the C ABI declared in
// include/fx_index.h: this file has the index's lifecycle (create, free,
// options, stream), add / reserve / reset, the file format, the profile and
// the calls that need no index; fx_api_*.cpp have one feature each, fx_plan.cpp
// the launch planners, fx_host.h what they share.  The index owns HBM (code
// matrix, row norms, search workspace), sequences the kernels on one HIP
// stream, and reproduces faiss's IndexFlatL2 API contract (faiss_store.py:29-128,
// rag_datastore_manager.py:138-218) at the C level.
#include "fx_host.h"

using namespace fx;

namespace {

thread_local std::string g_err;

// the labelled mode's buffer follows the rows' capacity (a no-op without
// labels, or when it is large enough): the ntotal labels are carried over
hipError_t grow_labels(FxIndex* h) {
    if (!h->has_ids || (h->idm.labels && (int64_t)(h->idm.labels.bytes / 8) >= h->cap_rows)) return hipSuccess;
    const int64_t cap = std::max<int64_t>(h->cap_rows, TILE_R);
    DevArr<int64_t> labels;  // (goes with the old buffer after the swap, or alone on an error)
    hipError_t e = labels.ensure((size_t)cap * 8);
    if (e != hipSuccess) return e;
    hipStream_t s = h->stream();
    if (h->idm.labels && h->ntotal > 0)
        e = hipMemcpyAsync(labels, h->idm.labels, (size_t)h->ntotal * 8, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // (searches in flight still read the old buffer)
    if (e != hipSuccess) return e;
    h->idm.labels.swap(labels);
    return hipSuccess;
}

hipError_t grow(FxIndex* h, int64_t need_rows) {
    if (need_rows <= h->cap_rows) return grow_labels(h);
    int64_t cap = round_up(std::max<int64_t>(need_rows, h->cap_rows + h->cap_rows / 2), TILE_R);
    DevArr<char> codes;  // the new arrays; after the swap the old ones, which go on return
    DevArr<float> norms;
    hipError_t e = codes.ensure((size_t)cap * h->row_bytes);
    if (e == hipSuccess) e = norms.ensure((size_t)cap * sizeof(float));
    if (e != hipSuccess) return e;
    hipStream_t s = h->stream();
    h->codes.swap(codes);
    h->norms.swap(norms);
    e = blank_rows(h, h->ntotal, cap, s);
    if (e == hipSuccess && h->ntotal > 0) {
        e = hipMemcpyAsync(h->codes, codes, (size_t)h->ntotal * h->row_bytes, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess)
            e = hipMemcpyAsync(h->norms, norms, (size_t)h->ntotal * sizeof(float), hipMemcpyDeviceToDevice, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {  // the index keeps its old arrays
        h->codes.swap(codes);
        h->norms.swap(norms);
        return e;
    }
    h->cap_rows = cap;
    return grow_labels(h);
}

}  // namespace

int fx::set_err(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

hipError_t fx::blank_rows(FxIndex* h, int64_t r0, int64_t r1, hipStream_t s) {
    hipError_t e = hipMemsetAsync(h->codes + (size_t)r0 * h->row_bytes, 0, (size_t)(r1 - r0) * h->row_bytes, s);
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)(h->norms + r0), 0x7f800000u, (size_t)(r1 - r0), s);
    return e;
}

hipError_t fx::stage_in(hipStream_t s, DevBuf& buf, const void* src, size_t bytes, int mem, const void** dev,
                        size_t offset) {
    *dev = src;
    if (mem != FX_MEM_HOST) return hipSuccess;
    hipError_t e = buf.ensure(std::max<size_t>(offset + bytes, 16));  // (never a null pointer for an empty input)
    if (e != hipSuccess) return e;
    *dev = (char*)buf.p + offset;
    return hipMemcpyAsync((char*)buf.p + offset, src, bytes, hipMemcpyHostToDevice, s);
}

extern "C" {

const char* fx_last_error(void) { return g_err.c_str(); }

int fx_device_count(int* out) {
    if (!out) return set_err(FX_E_ARG, "null out");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *out = 0;
        return set_err(FX_E_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *out = n;
    return FX_OK;
}

int fx_index_create(int d, int storage_dtype, int metric, int device, FxIndex** out) {
    if (!out) return set_err(FX_E_ARG, "null out");
    *out = nullptr;
    if (d <= 0) return set_err(FX_E_ARG, "dimension must be positive (got %d)", d);
    if (!check_dtype(storage_dtype)) return set_err(FX_E_ARG, "bad storage dtype %d", storage_dtype);
    if (metric != FX_METRIC_L2 && metric != FX_METRIC_INNER_PRODUCT)
        return set_err(FX_E_ARG, "bad metric %d", metric);
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return set_err(FX_E_HIP, "device %d not available (%d devices)", device, n);
    DeviceGuard g(device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", device);
    FxIndex* h = new FxIndex();
    h->d = d;
    h->dtype = storage_dtype;
    h->metric = metric;
    h->device = device;
    h->row_bytes = (int)round_up((int64_t)d * dtype_size(storage_dtype), ROW_ALIGN);
    h->kdim = h->row_bytes / dtype_size(storage_dtype);
    h->opt.from_env();
    // A BLOCKING stream: work on the legacy null stream (torch's default
    // stream, cuda_stream == 0) is ordered before and after it, so a caller
    // that binds "stream 0" (fx_index_set_stream(h, NULL)) stays ordered.
    hipError_t e = hipStreamCreateWithFlags(&h->own_stream, hipStreamDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->switch_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = h->max_sq_bits.ensure(16);
    if (e == hipSuccess) e = hipMemset(h->max_sq_bits, 0, 16);
    if (e == hipSuccess) e = h->dev_drop.ensure(16);
    if (e == hipSuccess) e = hipMemset(h->dev_drop, 0, 16);
    if (e != hipSuccess) {
        fx_index_free(h);
        return set_err(FX_E_HIP, "index init: %s", hipGetErrorString(e));
    }
    *out = h;
    return FX_OK;
}

void fx_index_free(FxIndex* h) {
    if (!h) return;
    DeviceGuard g(h->device);
    if (h->own_stream) (void)hipStreamSynchronize(h->own_stream);
    if (h->user_stream) (void)hipStreamSynchronize(h->user_stream);
    graph_release(h);
    for (hipEvent_t e : h->km.ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->km.ev_fin) (void)hipEventDestroy(e);
    for (auto& pr : h->ev_scan) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (auto& pr : h->ev_merge) (void)hipEventDestroy(pr.second);
    if (h->switch_ev) (void)hipEventDestroy(h->switch_ev);
    const hipStream_t own = h->own_stream;
    delete h;  // every buffer frees itself, with the index's device current and before its stream goes
    if (own) (void)hipStreamDestroy(own);
}

int fx_index_set_normalize(FxIndex* h, int on) {
    if (!h) return set_err(FX_E_ARG, "null index");
    std::lock_guard<std::mutex> lk(h->mu);
    h->normalize = on ? 1 : 0;
    return FX_OK;
}

int fx_index_set_stream(FxIndex* h, void* stream) {
    if (!h) return set_err(FX_E_ARG, "null index");
    std::lock_guard<std::mutex> lk(h->mu);
    const hipStream_t prev = h->stream();
    h->user_stream = (hipStream_t)stream;
    const hipStream_t next = h->stream();
    if (next != prev) {
        // the index's work stays in call order across a stream switch: the new
        // stream waits (on the device) for everything enqueued on the old one
        DeviceGuard g(h->device);
        HIP_TRY(hipEventRecord(h->switch_ev, prev));
        HIP_TRY(hipStreamWaitEvent(next, h->switch_ev, 0));
    }
    return FX_OK;
}

int fx_index_set_option(FxIndex* h, const char* name, int64_t value) {
    if (!h || !name) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (strcmp(name, "remove_stage") == 0) {  // (bytes: the one option wider than an int)
        if (value != 0 && (value < h->row_bytes || value > REMOVE_STAGE_MAX))
            return set_err(FX_E_ARG, "option 'remove_stage': value out of range (%lld; 0 or %d .. %lld bytes)",
                           (long long)value, h->row_bytes, (long long)REMOVE_STAGE_MAX);
        h->opt.remove_stage = value;
        return FX_OK;
    }
    const char* why = nullptr;
    int* slot = h->opt.find(name, value, &why);
    if (!slot) return set_err(FX_E_ARG, "unknown option '%s'", name);
    if (why) return set_err(FX_E_ARG, "option '%s': %s (%lld)", name, why, (long long)value);
    if (slot == &h->opt.range_cap && h->rg.cand.p) {
        // the next range search starts from the new capacity
        DeviceGuard g(h->device);
        HIP_TRY(hipStreamSynchronize(h->stream()));
        h->rg.cand.release();
    }
    *slot = (int)value;
    return FX_OK;
}

int fx_index_set_id_offset(FxIndex* h, int64_t off) {
    if (!h || off < 0) return set_err(FX_E_ARG, "bad index/offset");
    std::lock_guard<std::mutex> lk(h->mu);
    if (off != 0 && h->has_ids)
        return set_err(FX_E_ARG, "set_id_offset: the index carries labels (add_with_ids); ids are the labels, not row + offset");
    h->id_offset = off;
    return FX_OK;
}

int fx_index_dim(const FxIndex* h, int* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    *out = h->d;
    return FX_OK;
}
int fx_index_ntotal(const FxIndex* h, int64_t* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    *out = h->ntotal;
    return FX_OK;
}
int fx_index_storage_dtype(const FxIndex* h, int* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    *out = h->dtype;
    return FX_OK;
}
int fx_index_metric(const FxIndex* h, int* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    *out = h->metric;
    return FX_OK;
}

int fx_index_reserve(FxIndex* h, int64_t n) {
    if (!h || n < 0) return set_err(FX_E_ARG, "bad reserve");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    HIP_TRY(grow(h, n));
    return FX_OK;
}


}  // extern "C"

// the append of fx_index_add / fx_index_add_with_ids (arguments validated, the
// index locked): rows [ntotal, ntotal + n) <- x; ntotal is the caller's to advance
int fx::append_rows(FxIndex* h, int64_t n, const void* x, int x_dtype, int x_mem) {
    hipStream_t s = h->stream();
    HIP_TRY(grow(h, h->ntotal + n));
    const size_t xes = dtype_size(x_dtype);
    if (x_mem == FX_MEM_DEVICE) {
        HIP_TRY(launch_convert_rows(x, x_dtype, n, h->d, h->codes + (size_t)h->ntotal * h->row_bytes, h->dtype,
                                    h->kdim, h->norms + h->ntotal, h->max_sq_bits, h->normalize, s));
    } else {
        // stream host rows through a bounded staging buffer (<= 256 MiB)
        const int64_t chunk = std::max<int64_t>(1, (256ll << 20) / ((int64_t)h->d * xes));
        for (int64_t r0 = 0; r0 < n; r0 += chunk) {
            const int64_t nr = std::min(chunk, n - r0);
            HIP_TRY(h->stage.ensure((size_t)nr * h->d * xes));
            HIP_TRY(hipMemcpyAsync(h->stage.p, (const char*)x + (size_t)r0 * h->d * xes, (size_t)nr * h->d * xes,
                                   hipMemcpyHostToDevice, s));
            HIP_TRY(launch_convert_rows(h->stage.p, x_dtype, nr, h->d,
                                        h->codes + (size_t)(h->ntotal + r0) * h->row_bytes, h->dtype, h->kdim,
                                        h->norms + h->ntotal + r0, h->max_sq_bits, h->normalize, s));
            HIP_TRY(hipStreamSynchronize(s));  // staging buffer reuse
        }
    }
    return FX_OK;
}

int fx::check_add_args(const FxIndex* h, int64_t n, const void* x, int x_dtype) {
    if (!x) return set_err(FX_E_ARG, "null x");
    if (!check_dtype(x_dtype)) return set_err(FX_E_ARG, "bad x dtype %d", x_dtype);
    if ((int64_t)h->ntotal + n >= (int64_t)INT32_MAX) return set_err(FX_E_UNSUPPORTED, "more than 2^31-1 rows per shard");
    return FX_OK;
}

extern "C" {

int fx_index_add(FxIndex* h, int64_t n, const void* x, int x_dtype, int x_mem) {
    if (!h) return set_err(FX_E_ARG, "null index");
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (n == 0) return FX_OK;
    if (const int rc = check_add_args(h, n, x, x_dtype); rc != FX_OK) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->has_ids && h->ntotal > 0)
        return set_err(FX_E_ARG, "add does not make sense on an index with labels: use add_with_ids");
    h->has_ids = false;  // the first add into an empty index decides the mode
    DeviceGuard g(h->device);
    if (const int rc = append_rows(h, n, x, x_dtype, x_mem); rc != FX_OK) return rc;
    h->ntotal += n;
    return FX_OK;
}

int fx_index_reset(FxIndex* h) {
    if (!h) return set_err(FX_E_ARG, "null index");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream()));
    HIP_TRY(hipMemset(h->max_sq_bits, 0, 8));
    if (h->codes && h->cap_rows > 0) {
        HIP_TRY(blank_rows(h, 0, h->cap_rows, h->stream()));
        HIP_TRY(hipStreamSynchronize(h->stream()));
    }
    h->ntotal = 0;
    h->has_ids = false;  // the next add decides the mode again (the label buffer stays allocated)
    ++h->epoch;
    h->img_rows = 0;
    h->mu_rows = 0;
    h->rg.nq = -1;  // the last range search's result goes with the rows
    h->rg.total = 0;
    return FX_OK;
}

// the header fields an IxF2 file and an IxM2 / IxMp wrapper share, after the fourcc
static bool write_index_header(FILE* f, int32_t d, int64_t nt) {
    const int32_t metric = FX_METRIC_L2;
    const int64_t dummy = 1 << 20;
    const uint8_t trained = 1;
    return fwrite(&d, 4, 1, f) == 1 && fwrite(&nt, 8, 1, f) == 1 && fwrite(&dummy, 8, 1, f) == 1 &&
           fwrite(&dummy, 8, 1, f) == 1 && fwrite(&trained, 1, 1, f) == 1 && fwrite(&metric, 4, 1, f) == 1;
}
static bool read_index_header(FILE* f, int32_t* d, int64_t* nt, int32_t* metric) {
    int64_t d1 = 0, d2 = 0;
    uint8_t trained = 0;
    return fread(d, 4, 1, f) == 1 && fread(nt, 8, 1, f) == 1 && fread(&d1, 8, 1, f) == 1 && fread(&d2, 8, 1, f) == 1 &&
           fread(&trained, 1, 1, f) == 1 && fread(metric, 4, 1, f) == 1;
}

int fx_index_write(FxIndex* h, const char* path) {
    if (!h || !path) return set_err(FX_E_ARG, "null argument");
    if (h->metric != FX_METRIC_L2) return set_err(FX_E_UNSUPPORTED, "IxF2 writer supports METRIC_L2 only");
    FILE* f = fopen(path, "wb");
    if (!f) return set_err(FX_E_IO, "cannot open %s for writing", path);
    const int32_t d = h->d;
    const int64_t nt = h->ntotal, count = h->ntotal * (int64_t)h->d;
    const bool labelled = h->has_ids;
    bool ok = true;
    // a labelled index: faiss's IndexIDMap2 file -- its own header, the flat index as the sub-index, the labels
    if (labelled) ok = fwrite("IxM2", 1, 4, f) == 4 && write_index_header(f, d, nt);
    ok = ok && fwrite("IxF2", 1, 4, f) == 4 && write_index_header(f, d, nt) && fwrite(&count, 8, 1, f) == 1;
    const int64_t chunk = std::max<int64_t>(1, (64ll << 20) / ((int64_t)h->d * 4));
    std::vector<float> buf;
    for (int64_t r0 = 0; ok && r0 < nt; r0 += chunk) {
        const int64_t nr = std::min(chunk, nt - r0);
        buf.resize((size_t)nr * h->d);
        int rc = fx_index_reconstruct_n(h, r0, nr, buf.data());
        if (rc != FX_OK) {
            fclose(f);
            return rc;
        }
        ok = fwrite(buf.data(), 4, buf.size(), f) == buf.size();
    }
    if (ok && labelled) {
        std::vector<int64_t> ids((size_t)nt);
        const int rc = fx_index_get_ids(h, 0, nt, ids.data(), FX_MEM_HOST);
        if (rc != FX_OK) {
            fclose(f);
            return rc;
        }
        ok = fwrite(&nt, 8, 1, f) == 1 && fwrite(ids.data(), 8, ids.size(), f) == ids.size();
    }
    if (fclose(f) != 0) ok = false;
    if (!ok) return set_err(FX_E_IO, "short write to %s", path);
    return FX_OK;
}

int fx_index_read(const char* path, int storage_dtype, int device, FxIndex** out) {
    if (!path || !out) return set_err(FX_E_ARG, "null argument");
    *out = nullptr;
    FILE* f = fopen(path, "rb");
    if (!f) return set_err(FX_E_IO, "could not open %s for reading", path);
    char fourcc[4];
    int32_t d = 0, metric = 0;
    int64_t nt = 0, count = 0;
    bool ok = fread(fourcc, 1, 4, f) == 4;
    // IndexIDMap ("IxMp") / IndexIDMap2 ("IxM2"): a header of their own around the flat sub-index
    const bool labelled = ok && (memcmp(fourcc, "IxM2", 4) == 0 || memcmp(fourcc, "IxMp", 4) == 0);
    int32_t wd = 0, wmetric = 0;
    int64_t wnt = 0;
    if (labelled) ok = read_index_header(f, &wd, &wnt, &wmetric) && fread(fourcc, 1, 4, f) == 4;
    ok = ok && read_index_header(f, &d, &nt, &metric) && fread(&count, 8, 1, f) == 1;
    if (!ok) {
        fclose(f);
        return set_err(FX_E_IO, "%s: truncated IxF2 header", path);
    }
    if (memcmp(fourcc, "IxF2", 4) != 0) {
        fclose(f);
        return set_err(FX_E_IO, "%s: unsupported index fourcc (only IxF2 / IndexFlatL2, alone or inside IxMp / IxM2)", path);
    }
    if (d <= 0 || nt < 0 || metric != FX_METRIC_L2 || count != nt * (int64_t)d ||
        (labelled && (wd != d || wnt != nt || wmetric != metric))) {
        fclose(f);
        return set_err(FX_E_IO, "%s: inconsistent IxF2 header", path);
    }
    FxIndex* h = nullptr;
    int rc = fx_index_create(d, storage_dtype, FX_METRIC_L2, device, &h);
    if (rc != FX_OK) {
        fclose(f);
        return rc;
    }
    rc = fx_index_reserve(h, nt);
    const int64_t chunk = std::max<int64_t>(1, (64ll << 20) / ((int64_t)d * 4));
    std::vector<float> buf;
    for (int64_t r0 = 0; rc == FX_OK && r0 < nt; r0 += chunk) {
        const int64_t nr = std::min(chunk, nt - r0);
        buf.resize((size_t)nr * d);
        if (fread(buf.data(), 4, buf.size(), f) != buf.size()) {
            rc = set_err(FX_E_IO, "%s: truncated IxF2 codes", path);
            break;
        }
        rc = fx_index_add(h, nr, buf.data(), FX_F32, FX_MEM_HOST);
    }
    if (rc == FX_OK && labelled) {
        // i64 n, n labels: attached to the rows just added (the index becomes a labelled one)
        int64_t n = -1;
        std::vector<int64_t> ids;
        if (fread(&n, 8, 1, f) != 1 || n != nt) {
            rc = set_err(FX_E_IO, "%s: truncated or inconsistent id map (%lld ids for %lld rows)", path, (long long)n,
                         (long long)nt);
        } else {
            ids.resize((size_t)n);
            if (n > 0 && fread(ids.data(), 8, ids.size(), f) != ids.size()) rc = set_err(FX_E_IO, "%s: truncated id map", path);
        }
        if (rc == FX_OK) {
            std::lock_guard<std::mutex> lk(h->mu);
            DeviceGuard g(h->device);
            h->has_ids = true;
            hipError_t e = grow_labels(h);
            if (e == hipSuccess && n > 0) e = hipMemcpy(h->idm.labels, ids.data(), (size_t)n * 8, hipMemcpyHostToDevice);
            if (e != hipSuccess) rc = set_err(FX_E_HIP, "%s: storing the id map: %s", path, hipGetErrorString(e));
        }
    }
    fclose(f);
    if (rc != FX_OK) {
        fx_index_free(h);
        return rc;
    }
    *out = h;
    return FX_OK;
}

int fx_merge_shards(int metric, int nshards, int64_t nq, int k, const float* D_in, const int64_t* I_in, float* D_out,
                    int64_t* I_out, int device, void* stream) {
    if (nshards <= 0 || nq < 0 || k <= 0) return set_err(FX_E_ARG, "bad merge shape");
    if (!D_in || !I_in || !D_out || !I_out) return set_err(FX_E_ARG, "null buffer");
    if (metric != FX_METRIC_L2 && metric != FX_METRIC_INNER_PRODUCT) return set_err(FX_E_ARG, "bad metric");
    DeviceGuard g(device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", device);
    if (k > FX_MAX_K && nshards > FX_HUGEK_MAX_SHARDS)
        return set_err(FX_E_UNSUPPORTED, "merge of k = %d > %d lists supports at most %d shards (got %d)", k, FX_MAX_K,
                       FX_HUGEK_MAX_SHARDS, nshards);
    if (k > FX_MAX_K)  // stream-ordered sort merge (fx_hugek.hip)
        HIP_TRY(launch_merge_shards_sort(metric, nshards, nq, k, D_in, I_in, D_out, I_out, (hipStream_t)stream));
    else
        HIP_TRY(launch_merge_shards(metric, nshards, nq, k, D_in, I_in, D_out, I_out, (hipStream_t)stream));
    return FX_OK;
}

int fx_synth_fill(void* out, int64_t row0, int64_t n, int d, int dtype, uint64_t seed, int device, void* stream) {
    if (!out || n < 0 || d <= 0 || row0 < 0 || !check_dtype(dtype)) return set_err(FX_E_ARG, "bad synth args");
    DeviceGuard g(device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", device);
    HIP_TRY(launch_synth(out, row0, n, d, dtype, seed, (hipStream_t)stream));
    return FX_OK;
}

int fx_index_profile(FxIndex* h, int enable) {
    if (!h) return set_err(FX_E_ARG, "null index");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream()));
    for (auto& pr : h->ev_scan) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (auto& pr : h->ev_merge) (void)hipEventDestroy(pr.second);
    h->ev_scan.clear();
    h->ev_merge.clear();
    h->profile = enable != 0;
    return FX_OK;
}

int fx_index_profile_read(FxIndex* h, double* scan_ms, double* merge_ms, int64_t* launches) {
    if (!h || !scan_ms || !merge_ms || !launches) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream()));
    double a = 0, b = 0;
    for (size_t i = 0; i < h->ev_scan.size(); ++i) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev_scan[i].first, h->ev_scan[i].second));
        a += ms;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev_merge[i].first, h->ev_merge[i].second));
        b += ms;
    }
    *scan_ms = a;
    *merge_ms = b;
    *launches = (int64_t)h->ev_scan.size();
    return FX_OK;
}

}  // extern "C"

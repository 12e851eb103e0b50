// fx_api_sq.cpp -- scalar quantizer (fx_sq.hip): fx_sq_create / _train / _add / _search, the codec and the
// accessors.  The index owns its codes, row constants and tables; nothing of the flat index's state is shared.
// The handle, the row store and the search driver are the shared ones (fx_host.h, fx_flat_codes.h).
#include "fx_flat_codes.h"

using namespace fx;

namespace {

constexpr int QT_8BIT = 0, QT_8BIT_UNIFORM = 2;

// fx_sq_search's part of flat_codes_search
struct SqOps {
    static SqPlan plan(const FxSq* h, int64_t nq, int k) { return plan_sq(nq, h->ntotal, k, h->stride); }
    static hipError_t size(FxSq* h, int64_t, int64_t pad_max) {
        hipError_t e = h->qf32.ensure((size_t)pad_max * h->stride * 4);
        if (e == hipSuccess) e = h->planes.ensure((size_t)SQ_P * pad_max * h->stride);
        if (e == hipSuccess) e = h->sigma.ensure((size_t)pad_max * 4);
        return e;
    }
    // fp32 copies, the digit planes, the bound's terms
    static hipError_t prep(FxSq* h, const CodePass& ps) {
        SqPrep pp{};
        pp.q = ps.q;
        pp.q_dt = ps.q_dt;
        pp.metric = h->metric;
        pp.d = h->d;
        pp.row_bytes = h->stride;
        pp.nq = ps.nq;
        pp.nq_pad = ps.nq_pad;
        pp.trained = h->tables;
        pp.words = h->words;
        pp.qf32 = (float*)h->qf32.p;
        pp.planes = (char*)h->planes.p;
        pp.sigma = (float*)h->sigma.p;
        pp.qeps = (float*)h->eps.p;
        pp.qrho = (float*)h->rho.p;
        pp.qshift = (double*)h->shift.p;
        pp.zero[0] = ps.n_flag;
        pp.zero[1] = nullptr;
        return launch_sq_prep(pp, ps.s);
    }
    // the int8 MFMA scan
    static hipError_t scan(FxSq* h, const CodePass& ps) {
        SqScan sc{};
        sc.codes = h->codes;
        sc.nc = h->nc;
        sc.ntotal = h->ntotal;
        sc.row_bytes = h->stride;
        sc.planes = (char*)h->planes.p;
        sc.sigma = (float*)h->sigma.p;
        sc.nq = ps.nq;
        sc.nq_pad = ps.nq_pad;
        sc.n_qtiles = (int)(ps.nq_pad / TILE_Q);
        sc.n_ctiles = (int)((h->ntotal + TILE_R - 1) / TILE_R);
        sc.splits = ps.P->splits;
        sc.cand_d = (float*)h->cand_d.p;
        sc.cand_i = (int*)h->cand_i.p;
        return launch_sq_scan(h->metric, sc, ps.s);
    }
#ifdef FX_DIAG
    // FX_SQ_CAND: the pass's scan lists, query operands and the index's constants appended to the file:
    //   cand_d, cand_i [qtiles][splits][128][KP] | sigma [nq_pad] | qeps [nq] | qshift [nq] f64 |
    //   planes [3][nq_pad][row_bytes] | words [SQ_WORDS] | n_c [ntotal]
    static int dump(FxSq* h, const CodePass& ps) {
        const std::string& path = h->opt.sq_cand;
        if (path.empty()) return FX_OK;
        const size_t ncand = (size_t)(ps.nq_pad / TILE_Q) * ps.P->splits * TILE_Q * KP;
        HIP_TRY(hipStreamSynchronize(ps.s));
        HIP_TRY(dump_device<float>(path, h->cand_d.p, ncand));
        HIP_TRY(dump_device<int>(path, h->cand_i.p, ncand));
        HIP_TRY(dump_device<float>(path, h->sigma.p, (size_t)ps.nq_pad));
        HIP_TRY(dump_device<float>(path, h->eps.p, (size_t)ps.nq));
        HIP_TRY(dump_device<double>(path, h->shift.p, (size_t)ps.nq));
        HIP_TRY(dump_device<char>(path, h->planes.p, (size_t)SQ_P * ps.nq_pad * h->stride));
        HIP_TRY(dump_device<unsigned>(path, h->words, (size_t)SQ_WORDS));
        HIP_TRY(dump_device<float>(path, h->nc, (size_t)h->ntotal));
        return FX_OK;
    }
#endif
    static hipError_t refine(FxSq* h, const CodePass& ps) {
        SqRefine rp{};
        rp.cand_d = (float*)h->cand_d.p;
        rp.cand_i = (int*)h->cand_i.p;
        rp.splits = ps.P->splits;
        rp.nq = ps.nq;
        rp.ntotal = h->ntotal;
        rp.k = ps.k;
        rp.d = h->d;
        rp.row_bytes = h->stride;
        rp.codes = h->codes;
        rp.trained = h->tables;
        rp.words = h->words;
        rp.qf32 = (float*)h->qf32.p;
        rp.qeps = (float*)h->eps.p;
        rp.qshift = (double*)h->shift.p;
        rp.D = ps.D;
        rp.I = ps.I;
        rp.n_flag = ps.n_flag;
        rp.n_drop = h->cnt;
        rp.force_fb = h->opt.force_fallback != 0;
        return launch_sq_refine(h->metric, rp, ps.s);
    }
    static hipError_t exact(FxSq* h, const CodePass& ps) {
        SqExact ex{};
        ex.codes = h->codes;
        ex.row_bytes = h->stride;
        ex.d = h->d;
        ex.ntotal = h->ntotal;
        ex.trained = h->tables;
        ex.qf32 = (float*)h->qf32.p;
        ex.n_flag = ps.n_flag;
        ex.k = ps.k;
        ex.xs = ps.P->xsplits;
        ex.cd = (float*)h->cand_d.p;
        ex.ci = (int*)h->cand_i.p;
        ex.D = ps.D;
        ex.I = ps.I;
        return launch_sq_exact(h->metric, ex, ps.s);
    }
};

}  // namespace

extern "C" {

int fx_sq_create(int d, int qtype, int metric, int device, FxSq** out) {
    if (!out) return set_err(FX_E_ARG, "null out");
    *out = nullptr;
    if (d <= 0) return set_err(FX_E_ARG, "dimension must be positive (got %d)", d);
    if (qtype != QT_8BIT && qtype != QT_8BIT_UNIFORM)
        return set_err(FX_E_ARG, "sq: qtype %d is not offered (0 QT_8bit, 2 QT_8bit_uniform)", qtype);
    if (metric != FX_METRIC_L2 && metric != FX_METRIC_INNER_PRODUCT) return set_err(FX_E_ARG, "bad metric %d", metric);
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return set_err(FX_E_HIP, "device %d not available (%d devices)", device, n);
    DeviceGuard g(device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", device);
    FxSq* h = new FxSq();
    h->d = d;
    h->qtype = qtype;
    h->metric = metric;
    h->device = device;
    h->stride = (int)round_up(d, ROW_ALIGN);
    hipError_t e = h->init();
    if (e == hipSuccess) e = h->tables.ensure((size_t)2 * d * 4);
    if (e == hipSuccess) e = h->mm.ensure((size_t)2 * d * 4);
    if (e == hipSuccess) e = h->words.ensure(SQ_WORDS * 4);
    if (e == hipSuccess) e = hipMemset(h->words, 0, SQ_WORDS * 4);
    if (e == hipSuccess) e = h->bad.ensure(8);
    if (e == hipSuccess) e = hipMemset(h->bad, 0, 8);
    if (e != hipSuccess) {
        fx_sq_free(h);
        return set_err(FX_E_HIP, "sq init: %s", hipGetErrorString(e));
    }
    *out = h;
    return FX_OK;
}

void fx_sq_free(FxSq* h) { handle_free(h); }

int fx_sq_train(FxSq* h, int64_t n, const void* x, int x_dtype, int x_mem, int more) {
    if (const int rc = check_rows(n, x_dtype, x_mem); rc != FX_OK) return rc;
    if (!h) return set_err(FX_E_ARG, "null sq index");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->ntotal > 0) return set_err(FX_E_ARG, "sq train: the index holds %lld rows (reset it first)", (long long)h->ntotal);
    if (n == 0 && !h->train_open) return FX_OK;
    if (n > 0 && !x) return set_err(FX_E_ARG, "null x");
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    hipStream_t s = h->stream();
    if (!h->train_open) {
        HIP_TRY(launch_sq_minmax_reset(h->mm, h->d, h->bad, s));
        h->train_open = true;
        h->trained = false;
    }
    const int rc = staged_rows(s, h->in, n, x, (size_t)h->d * dtype_size(x_dtype), x_mem, 0,
                               [&](const void* xd, int64_t, int64_t nr) {
                                   HIP_TRY(launch_sq_minmax(xd, x_dtype, nr, h->d, h->mm, h->bad, s));
                                   return (int)FX_OK;
                               });
    if (rc != FX_OK || more) return rc;
    // the one synchronisation of a training: its non-finite count
    unsigned long long bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, h->bad, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    h->train_open = false;
    if (bad > 0) return set_err(FX_E_ARG, "sq train: %llu non-finite values in the training data", bad);
    HIP_TRY(launch_sq_finish(h->mm, h->d, h->qtype == QT_8BIT_UNIFORM, h->tables, s));
    HIP_TRY(launch_sq_consts(h->tables, h->d, h->words, s));
    h->trained = true;
    return FX_OK;
}

int fx_sq_is_trained(const FxSq* h, int* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    *out = h->trained ? 1 : 0;
    return FX_OK;
}

int fx_sq_get_trained(FxSq* h, float* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = need_trained(h->trained, "sq", "get_trained"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    return finish_out(h->stream(), out, h->tables, (size_t)2 * h->d * 4, FX_MEM_HOST);
}

int fx_sq_set_trained(FxSq* h, const float* trained) {
    if (!h || !trained) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->ntotal > 0)
        return set_err(FX_E_ARG, "sq set_trained: the index holds %lld rows (reset it first)", (long long)h->ntotal);
    if (const int rc = sq_check_tables("sq", h->d, trained); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    HIP_TRY(hipMemcpyAsync(h->tables, trained, (size_t)2 * h->d * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(launch_sq_consts(h->tables, h->d, h->words, s));
    h->train_open = false;
    h->trained = true;
    return FX_OK;
}

int fx_sq_add(FxSq* h, int64_t n, const void* x, int x_dtype, int x_mem) {
    if (const int rc = check_rows(n, x_dtype, x_mem); rc != FX_OK) return rc;
    if (!h) return set_err(FX_E_ARG, "null sq index");
    if (n == 0) return FX_OK;
    if (!x) return set_err(FX_E_ARG, "null x");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = need_trained(h->trained, "sq", "add"); rc != FX_OK) return rc;
    if (h->ntotal + n + 2 * TILE_R >= (int64_t)INT32_MAX) return set_err(FX_E_UNSUPPORTED, "sq: more than 2^31-1 rows");
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    hipStream_t s = h->stream();
    HIP_TRY(h->grow(h->ntotal + n, s));
    const int rc = staged_rows(s, h->in, n, x, (size_t)h->d * dtype_size(x_dtype), x_mem, 0,
                               [&](const void* xd, int64_t r0, int64_t nr) {
                                   const int64_t row0 = h->ntotal + r0;
                                   HIP_TRY(launch_sq_encode(xd, x_dtype, nr, h->d, h->tables, h->stride,
                                                            h->codes + (size_t)row0 * h->stride, h->nc + row0,
                                                            h->words, s));
                                   return (int)FX_OK;
                               });
    if (rc == FX_OK) h->ntotal += n;
    return rc;
}

int fx_sq_search(FxSq* h, int64_t nq, const void* q, int q_dtype, int q_mem, int k, float* D, int64_t* I, int out_mem) {
    return flat_codes_search<SqOps>(h, "sq", nq, q, q_dtype, q_mem, k, D, I, out_mem);
}

int fx_sq_reset(FxSq* h) {
    if (!h) return set_err(FX_E_ARG, "null sq index");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    HIP_TRY(hipStreamSynchronize(s));
    // the maxima restart; the decode bound belongs to the training and stays
    HIP_TRY(hipMemsetAsync(h->words, 0, 8, s));
    HIP_TRY(h->zero(s));
    h->ntotal = 0;
    h->clear_counts();
    return FX_OK;
}

int fx_sq_ntotal(const FxSq* h, int64_t* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    *out = h->ntotal;
    return FX_OK;
}

int fx_sq_reconstruct_batch(FxSq* h, int64_t n, const int64_t* keys, int keys_mem, float* out, int out_mem) {
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (!valid_mem(keys_mem) || !valid_mem(out_mem)) return set_err(FX_E_ARG, "bad keys_mem / out_mem");
    if (!h) return set_err(FX_E_ARG, "null sq index");
    if (n == 0) return FX_OK;
    if (!keys || !out) return set_err(FX_E_ARG, "null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = need_trained(h->trained, "sq", "reconstruct"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    const size_t bytes = (size_t)n * h->d * 4;
    const void* kd = nullptr;
    void* od = nullptr;
    HIP_TRY(stage_in(s, h->in, keys, (size_t)n * 8, keys_mem, &kd));
    HIP_TRY(out_buf(h->io, out, bytes, out_mem, &od));
    HIP_TRY(launch_sq_decode(h->codes, h->stride, 0, h->ntotal, (const int64_t*)kd, 0, n, h->d, h->tables, (float*)od, s));
    return finish_out(s, out, od, bytes, out_mem, keys_mem == FX_MEM_HOST);
}

int fx_sq_reconstruct_n(FxSq* h, int64_t i0, int64_t n, float* out, int out_mem) {
    if (n < 0 || i0 < 0) return set_err(FX_E_ARG, "negative i0 / n");
    if (!valid_mem(out_mem)) return set_err(FX_E_ARG, "bad out_mem %d", out_mem);
    if (!h) return set_err(FX_E_ARG, "null sq index");
    if (n == 0) return FX_OK;
    if (!out) return set_err(FX_E_ARG, "null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (i0 + n > h->ntotal)
        return set_err(FX_E_ARG, "sq reconstruct_n: rows [%lld, %lld) outside [0, %lld)", (long long)i0,
                       (long long)(i0 + n), (long long)h->ntotal);
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    const size_t bytes = (size_t)n * h->d * 4;
    void* od = nullptr;
    HIP_TRY(out_buf(h->io, out, bytes, out_mem, &od));
    HIP_TRY(launch_sq_decode(h->codes, h->stride, 0, h->ntotal, nullptr, i0, n, h->d, h->tables, (float*)od, s));
    return finish_out(s, out, od, bytes, out_mem);
}

int fx_sq_encode(FxSq* h, int64_t n, const void* x, int x_dtype, uint8_t* codes, int mem) {
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (!check_dtype(x_dtype)) return set_err(FX_E_ARG, "bad x dtype %d", x_dtype);
    if (!valid_mem(mem)) return set_err(FX_E_ARG, "bad mem %d", mem);
    if (!h) return set_err(FX_E_ARG, "null sq index");
    if (n == 0) return FX_OK;
    if (!x || !codes) return set_err(FX_E_ARG, "null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = need_trained(h->trained, "sq", "encode"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    const size_t bytes = (size_t)n * h->d;
    const void* xd = nullptr;
    void* od = nullptr;
    HIP_TRY(stage_in(s, h->in, x, (size_t)n * h->d * dtype_size(x_dtype), mem, &xd));
    HIP_TRY(out_buf(h->io, codes, bytes, mem, &od));
    HIP_TRY(launch_sq_encode_u8(xd, x_dtype, n, h->d, h->tables, (uint8_t*)od, s));
    return finish_out(s, codes, od, bytes, mem);
}

int fx_sq_decode(FxSq* h, int64_t n, const uint8_t* codes, float* out, int mem) {
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (!valid_mem(mem)) return set_err(FX_E_ARG, "bad mem %d", mem);
    if (!h) return set_err(FX_E_ARG, "null sq index");
    if (n == 0) return FX_OK;
    if (!codes || !out) return set_err(FX_E_ARG, "null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = need_trained(h->trained, "sq", "decode"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    const size_t bytes = (size_t)n * h->d * 4;
    const void* cd = nullptr;
    void* od = nullptr;
    HIP_TRY(stage_in(s, h->in, codes, (size_t)n * h->d, mem, &cd));
    HIP_TRY(out_buf(h->io, out, bytes, mem, &od));
    HIP_TRY(launch_sq_decode((const char*)cd, h->d, 0x80, n, nullptr, 0, n, h->d, h->tables, (float*)od, s));
    return finish_out(s, out, od, bytes, mem);
}

int fx_sq_set_stream(FxSq* h, void* stream) { return handle_set_stream(h, "sq", stream); }

int fx_sq_last_counts(FxSq* h, int64_t* fallbacks, int64_t* exact_fallbacks, int64_t* dropped) {
    return handle_last_counts(h, nullptr, fallbacks, exact_fallbacks, dropped);
}

int fx_sq_last_plan(FxSq* h, int* path, int* qtiles, int* splits, int* xsplits, int64_t* q_batch, int64_t* grid) {
    return flat_codes_last_plan(h, path, qtiles, splits, xsplits, q_batch, grid);
}

int fx_sq_profile(FxSq* h, int enable) { return handle_profile(h, "sq", enable); }

int fx_sq_profile_read(FxSq* h, double* prep_ms, double* scan_ms, double* refine_ms, int64_t* passes) {
    double* const ms[] = {prep_ms, scan_ms, refine_ms};
    return handle_profile_read(h, ms, passes);
}

}  // extern "C"

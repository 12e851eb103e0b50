// fx_api_sq.cpp -- scalar quantizer (fx_sq.hip): fx_sq_create / _train / _add / _search, the codec and the
// accessors.  The index owns its codes, row constants and tables; nothing of the flat index's state is shared.
#include "fx_host.h"
#include "fx_plan.h"

using namespace fx;

namespace {

constexpr int QT_8BIT = 0, QT_8BIT_UNIFORM = 2;

// Input of a call -> where the kernels read it (stage_in of fx_index.cpp, for this handle)
hipError_t sq_stage_in(FxSq* h, DevBuf& buf, const void* src, size_t bytes, int mem, const void** dev) {
    if (mem == FX_MEM_DEVICE) {
        *dev = src;
        return hipSuccess;
    }
    hipError_t e = buf.ensure(std::max<size_t>(bytes, 16));
    if (e != hipSuccess) return e;
    *dev = buf.p;
    return hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, h->stream());
}

// capacity for n rows and a whole tile past the last one; new rows hold code 0 and n_c = 0 (the scan masks
// rows at or past ntotal by row number)
hipError_t sq_grow(FxSq* h, int64_t n) {
    const int64_t want = round_up(n, TILE_R) + TILE_R;
    if (want <= h->cap_rows) return hipSuccess;
    const int64_t cap = std::max(want, round_up(h->cap_rows + h->cap_rows / 2, TILE_R));
    hipStream_t s = h->stream();
    DevBuf codes, nc;
    hipError_t e = codes.ensure((size_t)cap * h->row_bytes);
    if (e == hipSuccess) e = nc.ensure((size_t)cap * 4);
    if (e == hipSuccess) e = hipMemsetAsync(codes.p, 0, (size_t)cap * h->row_bytes, s);
    if (e == hipSuccess) e = hipMemsetAsync(nc.p, 0, (size_t)cap * 4, s);
    if (e == hipSuccess && h->ntotal > 0) {
        e = hipMemcpyAsync(codes.p, h->codes.p, (size_t)h->ntotal * h->row_bytes, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(nc.p, h->nc.p, (size_t)h->ntotal * 4, hipMemcpyDeviceToDevice, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // (work in flight still reads the old buffers)
    if (e != hipSuccess) return e;
    h->codes.swap(codes);
    h->nc.swap(nc);
    h->cap_rows = cap;
    return hipSuccess;
}

int sq_need_trained(const FxSq* h, const char* who) {
    if (!h->trained) return set_err(FX_E_ARG, "%s: the index is not trained", who);
    return FX_OK;
}

int sq_read_counts(FxSq* h) {
    if (h->counts_pending) {
        DeviceGuard g(h->device);
        HIP_TRY(hipStreamSynchronize(h->stream()));
        h->last_dropped = h->pin_cnt[0];
        h->last_fallbacks = h->pin_cnt[1];
        h->counts_pending = false;
    }
    return FX_OK;
}

// D / I of a search over an empty index
int sq_fill_missing(FxSq* h, int64_t nq, int k, float* D, int64_t* I, int out_mem) {
    const size_t n = (size_t)nq * k;
    std::vector<float> hd(n, h->metric == L2 ? FLT_MAX : -FLT_MAX);
    std::vector<int64_t> hi(n, -1);
    if (out_mem == FX_MEM_HOST) {
        memcpy(D, hd.data(), n * 4);
        memcpy(I, hi.data(), n * 8);
        return FX_OK;
    }
    hipStream_t s = h->stream();
    HIP_TRY(hipMemcpyAsync(D, hd.data(), n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(I, hi.data(), n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // (the host vectors go out of scope)
    return FX_OK;
}

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
    h->row_bytes = (int)round_up(d, ROW_ALIGN);
    h->opt.from_env();
    hipError_t e = hipStreamCreateWithFlags(&h->own_stream, hipStreamDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->switch_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = h->tables.ensure((size_t)2 * d * 4);
    if (e == hipSuccess) e = h->mm.ensure((size_t)2 * d * 4);
    if (e == hipSuccess) e = h->words.ensure(SQ_WORDS * 4);
    if (e == hipSuccess) e = hipMemset(h->words, 0, SQ_WORDS * 4);
    if (e == hipSuccess) e = h->bad.ensure(8);
    if (e == hipSuccess) e = hipMemset(h->bad, 0, 8);
    if (e == hipSuccess) e = h->cnt.ensure(16);
    if (e == hipSuccess) e = hipMemset(h->cnt, 0, 16);
    if (e == hipSuccess) e = h->pin_cnt.ensure(16);
    if (e != hipSuccess) {
        fx_sq_free(h);
        return set_err(FX_E_HIP, "sq init: %s", hipGetErrorString(e));
    }
    h->pin_cnt[0] = h->pin_cnt[1] = 0;
    *out = h;
    return FX_OK;
}

void fx_sq_free(FxSq* h) {
    if (!h) return;
    DeviceGuard g(h->device);
    if (h->own_stream) (void)hipStreamSynchronize(h->own_stream);
    if (h->user_stream) (void)hipStreamSynchronize(h->user_stream);
    for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
    if (h->switch_ev) (void)hipEventDestroy(h->switch_ev);
    const hipStream_t own = h->own_stream;
    delete h;  // its buffers, with the device current and before the stream goes
    if (own) (void)hipStreamDestroy(own);
}

int fx_sq_train(FxSq* h, int64_t n, const void* x, int x_dtype, int x_mem, int more) {
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (!check_dtype(x_dtype)) return set_err(FX_E_ARG, "bad x dtype %d", x_dtype);
    if (!valid_mem(x_mem)) return set_err(FX_E_ARG, "bad x_mem %d", x_mem);
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
    // host rows through a bounded staging buffer (<= 256 MiB)
    const size_t es = dtype_size(x_dtype);
    const int64_t chunk = x_mem == FX_MEM_DEVICE ? std::max<int64_t>(n, 1)
                                                 : std::max<int64_t>(1, (256ll << 20) / ((int64_t)h->d * es));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t nr = std::min(chunk, n - r0);
        const void* xd = nullptr;
        HIP_TRY(sq_stage_in(h, h->in, (const char*)x + (size_t)r0 * h->d * es, (size_t)nr * h->d * es, x_mem, &xd));
        HIP_TRY(launch_sq_minmax(xd, x_dtype, nr, h->d, h->mm, h->bad, s));
        if (x_mem == FX_MEM_HOST) HIP_TRY(hipStreamSynchronize(s));  // staging buffer reuse
    }
    if (more) return FX_OK;
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
    if (const int rc = sq_need_trained(h, "sq get_trained"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    HIP_TRY(hipMemcpyAsync(out, h->tables, (size_t)2 * h->d * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return FX_OK;
}

int fx_sq_set_trained(FxSq* h, const float* trained) {
    if (!h || !trained) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->ntotal > 0)
        return set_err(FX_E_ARG, "sq set_trained: the index holds %lld rows (reset it first)", (long long)h->ntotal);
    for (int j = 0; j < h->d; ++j)
        if (!std::isfinite(trained[j]) || !std::isfinite(trained[h->d + j]) || trained[h->d + j] < 0.f)
            return set_err(FX_E_ARG, "sq set_trained: dimension %d has vmin = %g, vdiff = %g", j, (double)trained[j],
                           (double)trained[h->d + j]);
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
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (!check_dtype(x_dtype)) return set_err(FX_E_ARG, "bad x dtype %d", x_dtype);
    if (!valid_mem(x_mem)) return set_err(FX_E_ARG, "bad x_mem %d", x_mem);
    if (!h) return set_err(FX_E_ARG, "null sq index");
    if (n == 0) return FX_OK;
    if (!x) return set_err(FX_E_ARG, "null x");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = sq_need_trained(h, "sq add"); rc != FX_OK) return rc;
    if (h->ntotal + n + 2 * TILE_R >= (int64_t)INT32_MAX) return set_err(FX_E_UNSUPPORTED, "sq: more than 2^31-1 rows");
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    hipStream_t s = h->stream();
    HIP_TRY(sq_grow(h, h->ntotal + n));
    const size_t es = dtype_size(x_dtype);
    const int64_t chunk = x_mem == FX_MEM_DEVICE ? n : std::max<int64_t>(1, (256ll << 20) / ((int64_t)h->d * es));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t nr = std::min(chunk, n - r0);
        const void* xd = nullptr;
        HIP_TRY(sq_stage_in(h, h->in, (const char*)x + (size_t)r0 * h->d * es, (size_t)nr * h->d * es, x_mem, &xd));
        HIP_TRY(launch_sq_encode(xd, x_dtype, nr, h->d, h->tables, h->row_bytes,
                                 h->codes + (size_t)(h->ntotal + r0) * h->row_bytes, h->nc + h->ntotal + r0, h->words, s));
        if (x_mem == FX_MEM_HOST) HIP_TRY(hipStreamSynchronize(s));  // staging buffer reuse
    }
    h->ntotal += n;
    return FX_OK;
}

int fx_sq_search(FxSq* h, int64_t nq, const void* q, int q_dtype, int q_mem, int k, float* D, int64_t* I, int out_mem) {
    if (nq < 0) return set_err(FX_E_ARG, "negative nq");
    if (k < 1) return set_err(FX_E_ARG, "k must be positive (got %d)", k);
    if (!check_dtype(q_dtype)) return set_err(FX_E_ARG, "bad query dtype %d", q_dtype);
    if (!valid_mem(q_mem) || !valid_mem(out_mem)) return set_err(FX_E_ARG, "bad q_mem / out_mem");
    if (k > FX_MAX_K) return set_err(FX_E_UNSUPPORTED, "sq search: k = %d above FX_MAX_K = %d", k, FX_MAX_K);
    if (!h) return set_err(FX_E_ARG, "null sq index");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = sq_need_trained(h, "sq search"); rc != FX_OK) return rc;
    if (nq == 0) return FX_OK;
    if (!q || !D || !I) return set_err(FX_E_ARG, "null buffer");
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    // (an earlier device search's counts, if nobody asked for them, give way to this search's)
    h->counts_pending = false;
    h->last_fallbacks = h->last_dropped = 0;
    if (h->ntotal == 0) return sq_fill_missing(h, nq, k, D, I, out_mem);

    hipStream_t s = h->stream();
    const SqPlan P = plan_sq(nq, h->ntotal, k, h->row_bytes);
    h->last_plan[0] = P.path;
    h->last_plan[1] = P.qtiles;
    h->last_plan[2] = P.splits;
    h->last_plan[3] = P.xsplits;
    h->last_qbatch = P.q_batch;
    h->last_grid = P.grid;
    const bool fused = P.path == SQ_PATH_FUSED;
    const int qes = dtype_size(q_dtype);
    const int rb = h->row_bytes;
    const void* qdev = nullptr;
    HIP_TRY(sq_stage_in(h, h->in, q, (size_t)nq * h->d * qes, q_mem, &qdev));
    const bool host_out = out_mem == FX_MEM_HOST;
    float* Dd = D;
    int64_t* Id = I;
    if (host_out) {
        HIP_TRY(h->outD.ensure((size_t)nq * k * 4));
        HIP_TRY(h->outI.ensure((size_t)nq * k * 8));
        Dd = (float*)h->outD.p;
        Id = (int64_t*)h->outI.p;
    }
    const int64_t qb_max = std::min(P.q_batch, nq);
    const int64_t pad_max = round_up(qb_max, QPAD);
    HIP_TRY(h->qf32.ensure((size_t)pad_max * rb * 4));
    HIP_TRY(h->planes.ensure((size_t)SQ_P * pad_max * rb));
    HIP_TRY(h->sigma.ensure((size_t)pad_max * 4));
    HIP_TRY(h->eps.ensure((size_t)qb_max * 4));
    HIP_TRY(h->rho.ensure((size_t)qb_max * 4));
    HIP_TRY(h->shift.ensure((size_t)qb_max * 8));
    HIP_TRY(h->flag.ensure((size_t)(qb_max + 1) * 4));
    HIP_TRY(h->cand_d.ensure((size_t)P.cand_bytes / 2));
    HIP_TRY(h->cand_i.ensure((size_t)P.cand_bytes / 2));
    HIP_TRY(hipMemsetAsync(h->cnt, 0, 16, s));
    int* n_flag = (int*)h->flag.p;

    for (int64_t q0 = 0; q0 < nq; q0 += qb_max) {
        const int64_t qb = std::min(qb_max, nq - q0);
        const int64_t nq_pad = round_up(qb, QPAD);
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        if (h->profile) {
            for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
            h->ev.insert(h->ev.end(), ev, ev + 4);
            HIP_TRY(hipEventRecord(ev[0], s));
        }
        // 1. query preparation: fp32 copies, the digit planes, the bound's terms; n_flag <- 0
        SqPrep pp{};
        pp.q = (const char*)qdev + (size_t)q0 * h->d * qes;
        pp.q_dt = q_dtype;
        pp.metric = h->metric;
        pp.d = h->d;
        pp.row_bytes = rb;
        pp.nq = qb;
        pp.nq_pad = nq_pad;
        pp.trained = h->tables;
        pp.words = h->words;
        pp.qf32 = (float*)h->qf32.p;
        pp.planes = (char*)h->planes.p;
        pp.sigma = (float*)h->sigma.p;
        pp.qeps = (float*)h->eps.p;
        pp.qrho = (float*)h->rho.p;
        pp.qshift = (double*)h->shift.p;
        pp.zero[0] = n_flag;
        pp.zero[1] = nullptr;
        HIP_TRY(launch_sq_prep(pp, s));
        if (h->profile) HIP_TRY(hipEventRecord(ev[1], s));
        SqExact ex{};
        ex.codes = h->codes;
        ex.row_bytes = rb;
        ex.d = h->d;
        ex.ntotal = h->ntotal;
        ex.trained = h->tables;
        ex.qf32 = pp.qf32;
        ex.n_flag = n_flag;
        ex.k = k;
        ex.xs = P.xsplits;
        ex.cd = (float*)h->cand_d.p;
        ex.ci = (int*)h->cand_i.p;
        ex.D = Dd + q0 * k;
        ex.I = Id + q0 * k;
        if (!fused) {
            // the exact path for the whole pass: every query "flagged"
            HIP_TRY(launch_ivf_flag_all(n_flag, qb, s));
            HIP_TRY(launch_sq_exact(h->metric, ex, s));
            if (h->profile) {  // (the exact scan is this path's "scan"; it has no refine)
                HIP_TRY(hipEventRecord(ev[2], s));
                HIP_TRY(hipEventRecord(ev[3], s));
            }
            continue;
        }
        // 2. the int8 MFMA scan: every (query tile, split) writes its sorted top-KP
        SqScan sc{};
        sc.codes = h->codes;
        sc.nc = h->nc;
        sc.ntotal = h->ntotal;
        sc.row_bytes = rb;
        sc.planes = pp.planes;
        sc.sigma = pp.sigma;
        sc.nq = qb;
        sc.nq_pad = nq_pad;
        sc.n_qtiles = (int)(nq_pad / TILE_Q);
        sc.n_ctiles = (int)((h->ntotal + TILE_R - 1) / TILE_R);
        sc.splits = P.splits;
        sc.cand_d = ex.cd;
        sc.cand_i = ex.ci;
        HIP_TRY(launch_sq_scan(h->metric, sc, s));
        if (h->profile) HIP_TRY(hipEventRecord(ev[2], s));
#ifdef FX_DIAG
        // FX_SQ_CAND: the pass's scan lists, query operands and the index's constants appended to the
        // file, before the refine reads the lists and the exact scan writes over them:
        //   cand_d, cand_i [qtiles][splits][128][KP] | sigma [nq_pad] | qeps [nq] | qshift [nq] f64 |
        //   planes [3][nq_pad][row_bytes] | words [SQ_WORDS] | n_c [ntotal]
        if (!h->opt.sq_cand.empty()) {
            const std::string& path = h->opt.sq_cand;
            const size_t ncand = (size_t)sc.n_qtiles * P.splits * TILE_Q * KP;
            HIP_TRY(hipStreamSynchronize(s));
            HIP_TRY(dump_device<float>(path, sc.cand_d, ncand));
            HIP_TRY(dump_device<int>(path, sc.cand_i, ncand));
            HIP_TRY(dump_device<float>(path, pp.sigma, (size_t)nq_pad));
            HIP_TRY(dump_device<float>(path, pp.qeps, (size_t)qb));
            HIP_TRY(dump_device<double>(path, pp.qshift, (size_t)qb));
            HIP_TRY(dump_device<char>(path, pp.planes, (size_t)SQ_P * nq_pad * rb));
            HIP_TRY(dump_device<unsigned>(path, h->words, (size_t)SQ_WORDS));
            HIP_TRY(dump_device<float>(path, h->nc, (size_t)h->ntotal));
        }
#endif
        // 3. refine + certification; every split pruned only with its own KP-th key
        SqRefine rp{};
        rp.cand_d = sc.cand_d;
        rp.cand_i = sc.cand_i;
        rp.splits = P.splits;
        rp.nq = qb;
        rp.ntotal = h->ntotal;
        rp.k = k;
        rp.d = h->d;
        rp.row_bytes = rb;
        rp.codes = h->codes;
        rp.trained = h->tables;
        rp.words = h->words;
        rp.qf32 = pp.qf32;
        rp.qeps = pp.qeps;
        rp.qshift = pp.qshift;
        rp.D = ex.D;
        rp.I = ex.I;
        rp.n_flag = n_flag;
        rp.n_drop = h->cnt;
        rp.force_fb = h->opt.force_fallback != 0;
        HIP_TRY(launch_sq_refine(h->metric, rp, s));
        // 4. the flagged queries' exact scan (device-gated; the candidate buffers are free again)
        HIP_TRY(launch_sq_exact(h->metric, ex, s));
        HIP_TRY(launch_ivf_accum(h->cnt + 1, n_flag, s));
        if (h->profile) HIP_TRY(hipEventRecord(ev[3], s));
    }
    HIP_TRY(hipMemcpyAsync(h->pin_cnt, h->cnt, 8, hipMemcpyDeviceToHost, s));
    h->counts_pending = true;
    if (!host_out) return FX_OK;
    HIP_TRY(hipMemcpyAsync(D, Dd, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(I, Id, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s));
    if (const int rc = sq_read_counts(h); rc != FX_OK) return rc;
    if (h->last_dropped > 0)
        return set_err(FX_E_INTEGRITY, "sq search: %lld candidate row ids outside [0, %lld) were dropped",
                       (long long)h->last_dropped, (long long)h->ntotal);
    return FX_OK;
}

int fx_sq_reset(FxSq* h) {
    if (!h) return set_err(FX_E_ARG, "null sq index");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    HIP_TRY(hipStreamSynchronize(s));
    // the maxima restart; the decode bound belongs to the training and stays
    HIP_TRY(hipMemsetAsync(h->words, 0, 8, s));
    if (h->cap_rows > 0) {
        HIP_TRY(hipMemsetAsync(h->codes, 0, (size_t)h->cap_rows * h->row_bytes, s));
        HIP_TRY(hipMemsetAsync(h->nc, 0, (size_t)h->cap_rows * 4, s));
    }
    h->ntotal = 0;
    h->counts_pending = false;
    h->last_fallbacks = h->last_dropped = 0;
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
    if (const int rc = sq_need_trained(h, "sq reconstruct"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    const void* kd = nullptr;
    HIP_TRY(sq_stage_in(h, h->in, keys, (size_t)n * 8, keys_mem, &kd));
    float* od = out;
    if (out_mem == FX_MEM_HOST) {
        HIP_TRY(h->io.ensure((size_t)n * h->d * 4));
        od = (float*)h->io.p;
    }
    HIP_TRY(launch_sq_decode(h->codes, h->row_bytes, 0, h->ntotal, (const int64_t*)kd, 0, n, h->d, h->tables, od, s));
    if (out_mem == FX_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(out, od, (size_t)n * h->d * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    } else if (keys_mem == FX_MEM_HOST) {
        HIP_TRY(hipStreamSynchronize(s));
    }
    return FX_OK;
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
    float* od = out;
    if (out_mem == FX_MEM_HOST) {
        HIP_TRY(h->io.ensure((size_t)n * h->d * 4));
        od = (float*)h->io.p;
    }
    HIP_TRY(launch_sq_decode(h->codes, h->row_bytes, 0, h->ntotal, nullptr, i0, n, h->d, h->tables, od, s));
    if (out_mem == FX_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(out, od, (size_t)n * h->d * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return FX_OK;
}

int fx_sq_encode(FxSq* h, int64_t n, const void* x, int x_dtype, uint8_t* codes, int mem) {
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (!check_dtype(x_dtype)) return set_err(FX_E_ARG, "bad x dtype %d", x_dtype);
    if (!valid_mem(mem)) return set_err(FX_E_ARG, "bad mem %d", mem);
    if (!h) return set_err(FX_E_ARG, "null sq index");
    if (n == 0) return FX_OK;
    if (!x || !codes) return set_err(FX_E_ARG, "null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = sq_need_trained(h, "sq encode"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    const void* xd = nullptr;
    HIP_TRY(sq_stage_in(h, h->in, x, (size_t)n * h->d * dtype_size(x_dtype), mem, &xd));
    uint8_t* od = codes;
    if (mem == FX_MEM_HOST) {
        HIP_TRY(h->io.ensure((size_t)n * h->d));
        od = (uint8_t*)h->io.p;
    }
    HIP_TRY(launch_sq_encode_u8(xd, x_dtype, n, h->d, h->tables, od, s));
    if (mem == FX_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(codes, od, (size_t)n * h->d, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return FX_OK;
}

int fx_sq_decode(FxSq* h, int64_t n, const uint8_t* codes, float* out, int mem) {
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (!valid_mem(mem)) return set_err(FX_E_ARG, "bad mem %d", mem);
    if (!h) return set_err(FX_E_ARG, "null sq index");
    if (n == 0) return FX_OK;
    if (!codes || !out) return set_err(FX_E_ARG, "null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = sq_need_trained(h, "sq decode"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    const void* cd = nullptr;
    HIP_TRY(sq_stage_in(h, h->in, codes, (size_t)n * h->d, mem, &cd));
    float* od = out;
    if (mem == FX_MEM_HOST) {
        HIP_TRY(h->io.ensure((size_t)n * h->d * 4));
        od = (float*)h->io.p;
    }
    HIP_TRY(launch_sq_decode((const char*)cd, h->d, 0x80, n, nullptr, 0, n, h->d, h->tables, od, s));
    if (mem == FX_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(out, od, (size_t)n * h->d * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return FX_OK;
}

int fx_sq_set_stream(FxSq* h, void* stream) {
    if (!h) return set_err(FX_E_ARG, "null sq index");
    std::lock_guard<std::mutex> lk(h->mu);
    const hipStream_t prev = h->stream();
    h->user_stream = (hipStream_t)stream;
    const hipStream_t next = h->stream();
    if (next != prev) {
        DeviceGuard g(h->device);
        HIP_TRY(hipEventRecord(h->switch_ev, prev));
        HIP_TRY(hipStreamWaitEvent(next, h->switch_ev, 0));
    }
    return FX_OK;
}

int fx_sq_last_counts(FxSq* h, int64_t* fallbacks, int64_t* exact_fallbacks, int64_t* dropped) {
    if (!h || !fallbacks || !exact_fallbacks || !dropped) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = sq_read_counts(h); rc != FX_OK) return rc;
    *fallbacks = h->last_fallbacks;
    *exact_fallbacks = h->last_fallbacks;
    *dropped = h->last_dropped;
    return FX_OK;
}

int fx_sq_last_plan(FxSq* h, int* path, int* qtiles, int* splits, int* xsplits, int64_t* q_batch, int64_t* grid) {
    if (!h || !path || !qtiles || !splits || !xsplits || !q_batch || !grid) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *path = h->last_plan[0];
    *qtiles = h->last_plan[1];
    *splits = h->last_plan[2];
    *xsplits = h->last_plan[3];
    *q_batch = h->last_qbatch;
    *grid = h->last_grid;
    return FX_OK;
}

int fx_sq_profile(FxSq* h, int enable) {
    if (!h) return set_err(FX_E_ARG, "null sq index");
    std::lock_guard<std::mutex> lk(h->mu);
    h->profile = enable != 0;
    return FX_OK;
}

int fx_sq_profile_read(FxSq* h, double* prep_ms, double* scan_ms, double* refine_ms, int64_t* passes) {
    if (!h || !prep_ms || !scan_ms || !refine_ms || !passes) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    HIP_TRY(hipStreamSynchronize(h->stream()));
    double ms[3] = {0, 0, 0};
    float t = 0;
    for (size_t i = 0; i + 3 < h->ev.size(); i += 4)
        for (int part = 0; part < 3; ++part) {
            HIP_TRY(hipEventElapsedTime(&t, h->ev[i + part], h->ev[i + part + 1]));
            ms[part] += t;
        }
    *passes = (int64_t)(h->ev.size() / 4);
    for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
    h->ev.clear();
    *prep_ms = ms[0];
    *scan_ms = ms[1];
    *refine_ms = ms[2];
    return FX_OK;
}

}  // extern "C"

// fx_api_pq.cpp -- product quantizer (fx_pq.hip): fx_pq_create / _set_centroids / _add / _search, the codec and
// the accessors.  The index owns its codes, row constants, centroids and their scan image; nothing of the flat
// index's state is shared.  Training is the caller's (M k-means runs, the Python layer): the centroids arrive
// through fx_pq_set_centroids, which rebuilds the scan image and the bound's constants on the host.
#include "fx_host.h"
#include "fx_plan.h"

using namespace fx;

namespace {

// bf16 round to nearest even (finite input), as the device's f2bf
uint16_t host_f2bf(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
float host_bf2f(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

hipError_t pq_stage_in(FxPq* h, DevBuf& buf, const void* src, size_t bytes, int mem, const void** dev) {
    if (mem == FX_MEM_DEVICE) {
        *dev = src;
        return hipSuccess;
    }
    hipError_t e = buf.ensure(std::max<size_t>(bytes, 16));
    if (e != hipSuccess) return e;
    *dev = buf.p;
    return hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, h->stream());
}

// capacity for n rows and a whole tile past the last one; new rows hold code 0 and n_y = 0 (the scan forms
// gather addresses from them, which code 0 keeps inside the image, and masks them by row number)
hipError_t pq_grow(FxPq* h, int64_t n) {
    const int64_t want = round_up(n, TILE_R) + TILE_R;
    if (want <= h->cap_rows) return hipSuccess;
    const int64_t cap = std::max(want, round_up(h->cap_rows + h->cap_rows / 2, TILE_R));
    hipStream_t s = h->stream();
    DevBuf codes, ny;
    hipError_t e = codes.ensure((size_t)cap * h->stride);
    if (e == hipSuccess) e = ny.ensure((size_t)cap * 4);
    if (e == hipSuccess) e = hipMemsetAsync(codes.p, 0, (size_t)cap * h->stride, s);
    if (e == hipSuccess) e = hipMemsetAsync(ny.p, 0, (size_t)cap * 4, s);
    if (e == hipSuccess && h->ntotal > 0) {
        e = hipMemcpyAsync(codes.p, h->codes.p, (size_t)h->ntotal * h->stride, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(ny.p, h->ny.p, (size_t)h->ntotal * 4, hipMemcpyDeviceToDevice, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // (work in flight still reads the old buffers)
    if (e != hipSuccess) return e;
    h->codes.swap(codes);
    h->ny.swap(ny);
    h->cap_rows = cap;
    return hipSuccess;
}

int pq_need_trained(const FxPq* h, const char* who) {
    if (!h->trained) return set_err(FX_E_ARG, "%s: the index is not trained", who);
    return FX_OK;
}

int pq_read_counts(FxPq* h) {
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
int pq_fill_missing(FxPq* h, int64_t nq, int k, float* D, int64_t* I, int out_mem) {
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

int fx_pq_create(int d, int M, int nbits, int metric, int device, FxPq** out) {
    if (!out) return set_err(FX_E_ARG, "null out");
    *out = nullptr;
    if (d <= 0) return set_err(FX_E_ARG, "dimension must be positive (got %d)", d);
    if (M <= 0 || M > 65535 || d % M != 0)
        return set_err(FX_E_ARG, "pq: d = %d is not a multiple of M = %d (1 <= M <= 65535)", d, M);
    if (nbits != 8) return set_err(FX_E_UNSUPPORTED, "pq: nbits = %d is not offered (8)", nbits);
    if (metric != FX_METRIC_L2 && metric != FX_METRIC_INNER_PRODUCT) return set_err(FX_E_ARG, "bad metric %d", metric);
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return set_err(FX_E_HIP, "device %d not available (%d devices)", device, n);
    DeviceGuard g(device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", device);
    FxPq* h = new FxPq();
    h->d = d;
    h->M = M;
    h->dsub = d / M;
    h->metric = metric;
    h->device = device;
    h->stride = pq_stride(M);
    h->kp = pq_kpad(d);
    h->opt.from_env();
    const size_t cb_bytes = (size_t)M * PQ_KSUB * h->dsub * 4;
    hipError_t e = hipStreamCreateWithFlags(&h->own_stream, hipStreamDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->switch_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = h->cb.ensure(cb_bytes);
    if (e == hipSuccess && h->dsub % 8 == 0) e = h->img.ensure((size_t)2 * pq_plane_bytes(M, h->dsub));
    if (e == hipSuccess) e = h->cnt.ensure(16);
    if (e == hipSuccess) e = hipMemset(h->cnt, 0, 16);
    if (e == hipSuccess) e = h->pin_cnt.ensure(16);
    if (e != hipSuccess) {
        fx_pq_free(h);
        return set_err(FX_E_HIP, "pq init: %s", hipGetErrorString(e));
    }
    h->pin_cnt[0] = h->pin_cnt[1] = 0;
    *out = h;
    return FX_OK;
}

void fx_pq_free(FxPq* h) {
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

int fx_pq_is_trained(const FxPq* h, int* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    *out = h->trained ? 1 : 0;
    return FX_OK;
}

int fx_pq_get_centroids(FxPq* h, float* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = pq_need_trained(h, "pq get_centroids"); rc != FX_OK) return rc;
    memcpy(out, h->h_cb.data(), h->h_cb.size() * 4);
    return FX_OK;
}

int fx_pq_set_centroids(FxPq* h, const float* centroids) {
    if (!h || !centroids) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->ntotal > 0)
        return set_err(FX_E_ARG, "pq set_centroids: the index holds %lld rows (reset it first)", (long long)h->ntotal);
    const int M = h->M, dsub = h->dsub;
    const size_t nval = (size_t)M * PQ_KSUB * dsub;
    for (size_t i = 0; i < nval; ++i)
        if (!std::isfinite(centroids[i]))
            return set_err(FX_E_ARG, "pq set_centroids: centroid %lld of sub-quantizer %lld has a non-finite value",
                           (long long)(i / dsub % PQ_KSUB), (long long)(i / dsub / PQ_KSUB));
    // the bound's constants: per sub-quantizer maxima, so they hold for any code row; the scan image
    const bool scan = dsub % 8 == 0;
    const size_t plane = (size_t)pq_plane_bytes(M, dsub) / 2;  // bf16 values of a plane
    std::vector<uint16_t> img(scan ? 2 * plane : 0, 0);
    double y2 = 0.0, r2 = 0.0, l2 = 0.0;
    for (int m = 0; m < M; ++m) {
        double my = 0.0, mr = 0.0, ml = 0.0;
        for (int j = 0; j < PQ_KSUB; ++j) {
            double sy = 0.0, sr = 0.0, sl = 0.0;
            for (int e = 0; e < dsub; ++e) {
                const size_t i = ((size_t)m * PQ_KSUB + j) * dsub + e;
                const float v = centroids[i];
                const uint16_t hb = host_f2bf(v);
                const float rest = v - host_bf2f(hb);  // exact in fp32
                const uint16_t lb = std::isfinite(host_bf2f(hb)) ? host_f2bf(rest) : (uint16_t)0;
                const double lo = (double)host_bf2f(lb), res = (double)rest - lo;
                sy += (double)v * (double)v;
                sr += res * res;
                sl += lo * lo;
                if (scan) {
                    img[i] = hb;
                    img[plane + i] = lb;
                }
            }
            my = std::max(my, sy);
            mr = std::max(mr, sr);
            ml = std::max(ml, sl);
        }
        y2 += my;
        r2 += mr;
        l2 += ml;
    }
    if (!std::isfinite(y2) || !std::isfinite(r2) || !(y2 < 1e37))
        return set_err(FX_E_ARG, "pq set_centroids: the centroids' norms leave the fp32 range");
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    hipStream_t s = h->stream();
    HIP_TRY(hipStreamSynchronize(s));  // (an earlier search may still read the image)
    HIP_TRY(hipMemcpyAsync(h->cb, centroids, nval * 4, hipMemcpyHostToDevice, s));
    if (scan) HIP_TRY(hipMemcpyAsync(h->img, img.data(), img.size() * 2, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    h->h_cb.assign(centroids, centroids + nval);
    const double up = 1.0 + 1e-9;
    h->Y = std::sqrt(y2) * up;
    h->Ry = std::sqrt(r2) * up;
    h->Yl = std::sqrt(l2) * up;
    h->trained = true;
    return FX_OK;
}

int fx_pq_add(FxPq* h, int64_t n, const void* x, int x_dtype, int x_mem) {
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (!check_dtype(x_dtype)) return set_err(FX_E_ARG, "bad x dtype %d", x_dtype);
    if (!valid_mem(x_mem)) return set_err(FX_E_ARG, "bad x_mem %d", x_mem);
    if (!h) return set_err(FX_E_ARG, "null pq index");
    if (n == 0) return FX_OK;
    if (!x) return set_err(FX_E_ARG, "null x");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = pq_need_trained(h, "pq add"); rc != FX_OK) return rc;
    if (h->ntotal + n + 2 * TILE_R >= (int64_t)INT32_MAX) return set_err(FX_E_UNSUPPORTED, "pq: more than 2^31-1 rows");
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    hipStream_t s = h->stream();
    HIP_TRY(pq_grow(h, h->ntotal + n));
    const size_t es = dtype_size(x_dtype);
    const int64_t chunk = x_mem == FX_MEM_DEVICE ? n : std::max<int64_t>(1, (256ll << 20) / ((int64_t)h->d * es));
    for (int64_t r0 = 0; r0 < n; r0 += chunk) {
        const int64_t nr = std::min(chunk, n - r0);
        const void* xd = nullptr;
        HIP_TRY(pq_stage_in(h, h->in, (const char*)x + (size_t)r0 * h->d * es, (size_t)nr * h->d * es, x_mem, &xd));
        uint8_t* c0 = h->codes + (size_t)(h->ntotal + r0) * h->stride;
        HIP_TRY(launch_pq_encode(xd, x_dtype, nr, h->d, h->M, h->dsub, h->cb, c0, h->stride, s));
        HIP_TRY(launch_pq_ny(c0, h->stride, nr, h->M, h->dsub, h->cb, h->ny + h->ntotal + r0, s));
        if (x_mem == FX_MEM_HOST) HIP_TRY(hipStreamSynchronize(s));  // staging buffer reuse
    }
    h->ntotal += n;
    return FX_OK;
}

int fx_pq_search(FxPq* h, int64_t nq, const void* q, int q_dtype, int q_mem, int k, float* D, int64_t* I, int out_mem) {
    if (nq < 0) return set_err(FX_E_ARG, "negative nq");
    if (k < 1) return set_err(FX_E_ARG, "k must be positive (got %d)", k);
    if (!check_dtype(q_dtype)) return set_err(FX_E_ARG, "bad query dtype %d", q_dtype);
    if (!valid_mem(q_mem) || !valid_mem(out_mem)) return set_err(FX_E_ARG, "bad q_mem / out_mem");
    if (k > FX_MAX_K) return set_err(FX_E_UNSUPPORTED, "pq search: k = %d above FX_MAX_K = %d", k, FX_MAX_K);
    if (!h) return set_err(FX_E_ARG, "null pq index");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = pq_need_trained(h, "pq search"); rc != FX_OK) return rc;
    if (nq == 0) return FX_OK;
    if (!q || !D || !I) return set_err(FX_E_ARG, "null buffer");
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    // (an earlier device search's counts, if nobody asked for them, give way to this search's)
    h->counts_pending = false;
    h->last_fallbacks = h->last_dropped = 0;
    if (h->ntotal == 0) return pq_fill_missing(h, nq, k, D, I, out_mem);

    hipStream_t s = h->stream();
    const SqPlan P = plan_pq(nq, h->ntotal, k, h->M, h->dsub);
    h->last_plan[0] = P.path;
    h->last_plan[1] = P.qtiles;
    h->last_plan[2] = P.splits;
    h->last_plan[3] = P.xsplits;
    h->last_qbatch = P.q_batch;
    h->last_grid = P.grid;
    const bool fused = P.path == SQ_PATH_FUSED;
    const int qes = dtype_size(q_dtype);
    const int kp = h->kp;
    const void* qdev = nullptr;
    HIP_TRY(pq_stage_in(h, h->in, q, (size_t)nq * h->d * qes, q_mem, &qdev));
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
    HIP_TRY(h->qf32.ensure((size_t)pad_max * kp * 4));
    HIP_TRY(h->planes.ensure((size_t)2 * pad_max * kp * 2));
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
        // 1. query preparation: fp32 copies, the [hi | lo] planes, the bound; n_flag <- 0
        PqPrep pp{};
        pp.q = (const char*)qdev + (size_t)q0 * h->d * qes;
        pp.q_dt = q_dtype;
        pp.metric = h->metric;
        pp.d = h->d;
        pp.kp = kp;
        pp.nq = qb;
        pp.nq_pad = nq_pad;
        pp.Y = h->Y;
        pp.Ry = h->Ry;
        pp.Yl = h->Yl;
        pp.qf32 = (float*)h->qf32.p;
        pp.planes = (uint16_t*)h->planes.p;
        pp.qeps = (float*)h->eps.p;
        pp.qrho = (float*)h->rho.p;
        pp.qshift = (double*)h->shift.p;
        pp.zero[0] = n_flag;
        pp.zero[1] = nullptr;
        HIP_TRY(launch_pq_prep(pp, s));
        if (h->profile) HIP_TRY(hipEventRecord(ev[1], s));
        PqExact ex{};
        ex.codes = h->codes;
        ex.stride = h->stride;
        ex.M = h->M;
        ex.dsub = h->dsub;
        ex.d = h->d;
        ex.kp = kp;
        ex.ntotal = h->ntotal;
        ex.cb = h->cb;
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
            HIP_TRY(launch_pq_exact(h->metric, ex, s));
            if (h->profile) {  // (the exact scan is this path's "scan"; it has no refine)
                HIP_TRY(hipEventRecord(ev[2], s));
                HIP_TRY(hipEventRecord(ev[3], s));
            }
            continue;
        }
        // 2. the gather scan: every (query tile, split) writes its sorted top-KP
        PqScan sc{};
        sc.codes = h->codes;
        sc.ny = h->ny;
        sc.ntotal = h->ntotal;
        sc.stride = h->stride;
        sc.M = h->M;
        sc.dsub = h->dsub;
        sc.d = h->d;
        sc.kp = kp;
        sc.img = h->img;
        sc.plane_bytes = pq_plane_bytes(h->M, h->dsub);
        sc.planes = pp.planes;
        sc.nq = qb;
        sc.nq_pad = nq_pad;
        sc.n_qtiles = (int)(nq_pad / TILE_Q);
        sc.n_ctiles = (int)((h->ntotal + TILE_R - 1) / TILE_R);
        sc.splits = P.splits;
        sc.cand_d = ex.cd;
        sc.cand_i = ex.ci;
        HIP_TRY(launch_pq_scan(h->metric, sc, s));
        if (h->profile) HIP_TRY(hipEventRecord(ev[2], s));
#ifdef FX_DIAG
        // FX_PQ_CAND: the pass's scan lists, query operands and the rows' constants appended to the file,
        // before the refine reads the lists and the exact scan writes over them:
        //   cand_d, cand_i [qtiles][splits][128][KP] | qeps [nq] | qshift [nq] f64 |
        //   planes [2][nq_pad][kp] bf16 | codes [ntotal][stride] u8 | n_y [ntotal]
        if (!h->opt.pq_cand.empty()) {
            const std::string& path = h->opt.pq_cand;
            const size_t ncand = (size_t)sc.n_qtiles * P.splits * TILE_Q * KP;
            HIP_TRY(hipStreamSynchronize(s));
            HIP_TRY(dump_device<float>(path, sc.cand_d, ncand));
            HIP_TRY(dump_device<int>(path, sc.cand_i, ncand));
            HIP_TRY(dump_device<float>(path, pp.qeps, (size_t)qb));
            HIP_TRY(dump_device<double>(path, pp.qshift, (size_t)qb));
            HIP_TRY(dump_device<uint16_t>(path, pp.planes, (size_t)2 * nq_pad * kp));
            HIP_TRY(dump_device<uint8_t>(path, h->codes, (size_t)h->ntotal * h->stride));
            HIP_TRY(dump_device<float>(path, h->ny, (size_t)h->ntotal));
        }
#endif
        // 3. refine + certification; every split pruned only with its own KP-th key
        PqRefine rp{};
        rp.cand_d = sc.cand_d;
        rp.cand_i = sc.cand_i;
        rp.splits = P.splits;
        rp.nq = qb;
        rp.ntotal = h->ntotal;
        rp.k = k;
        rp.d = h->d;
        rp.kp = kp;
        rp.M = h->M;
        rp.dsub = h->dsub;
        rp.stride = h->stride;
        rp.codes = h->codes;
        rp.cb = h->cb;
        rp.qf32 = pp.qf32;
        rp.qeps = pp.qeps;
        rp.qshift = pp.qshift;
        rp.D = ex.D;
        rp.I = ex.I;
        rp.n_flag = n_flag;
        rp.n_drop = h->cnt;
        rp.force_fb = h->opt.force_fallback != 0;
        HIP_TRY(launch_pq_refine(h->metric, rp, s));
        // 4. the flagged queries' exact scan (device-gated; the candidate buffers are free again)
        HIP_TRY(launch_pq_exact(h->metric, ex, s));
        HIP_TRY(launch_ivf_accum(h->cnt + 1, n_flag, s));
        if (h->profile) HIP_TRY(hipEventRecord(ev[3], s));
    }
    HIP_TRY(hipMemcpyAsync(h->pin_cnt, h->cnt, 8, hipMemcpyDeviceToHost, s));
    h->counts_pending = true;
    if (!host_out) return FX_OK;
    HIP_TRY(hipMemcpyAsync(D, Dd, (size_t)nq * k * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(I, Id, (size_t)nq * k * 8, hipMemcpyDeviceToHost, s));
    if (const int rc = pq_read_counts(h); rc != FX_OK) return rc;
    if (h->last_dropped > 0)
        return set_err(FX_E_INTEGRITY, "pq search: %lld candidate row ids outside [0, %lld) were dropped",
                       (long long)h->last_dropped, (long long)h->ntotal);
    return FX_OK;
}

int fx_pq_reset(FxPq* h) {
    if (!h) return set_err(FX_E_ARG, "null pq index");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    HIP_TRY(hipStreamSynchronize(s));
    if (h->cap_rows > 0) {
        HIP_TRY(hipMemsetAsync(h->codes, 0, (size_t)h->cap_rows * h->stride, s));
        HIP_TRY(hipMemsetAsync(h->ny, 0, (size_t)h->cap_rows * 4, s));
    }
    h->ntotal = 0;
    h->counts_pending = false;
    h->last_fallbacks = h->last_dropped = 0;
    return FX_OK;
}

int fx_pq_ntotal(const FxPq* h, int64_t* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    *out = h->ntotal;
    return FX_OK;
}

int fx_pq_reconstruct_batch(FxPq* h, int64_t n, const int64_t* keys, int keys_mem, float* out, int out_mem) {
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (!valid_mem(keys_mem) || !valid_mem(out_mem)) return set_err(FX_E_ARG, "bad keys_mem / out_mem");
    if (!h) return set_err(FX_E_ARG, "null pq index");
    if (n == 0) return FX_OK;
    if (!keys || !out) return set_err(FX_E_ARG, "null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = pq_need_trained(h, "pq reconstruct"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    const void* kd = nullptr;
    HIP_TRY(pq_stage_in(h, h->in, keys, (size_t)n * 8, keys_mem, &kd));
    float* od = out;
    if (out_mem == FX_MEM_HOST) {
        HIP_TRY(h->io.ensure((size_t)n * h->d * 4));
        od = (float*)h->io.p;
    }
    HIP_TRY(launch_pq_decode(h->codes, h->stride, h->ntotal, (const int64_t*)kd, 0, n, h->M, h->dsub, h->cb, od, s));
    if (out_mem == FX_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(out, od, (size_t)n * h->d * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    } else if (keys_mem == FX_MEM_HOST) {
        HIP_TRY(hipStreamSynchronize(s));
    }
    return FX_OK;
}

int fx_pq_reconstruct_n(FxPq* h, int64_t i0, int64_t n, float* out, int out_mem) {
    if (n < 0 || i0 < 0) return set_err(FX_E_ARG, "negative i0 / n");
    if (!valid_mem(out_mem)) return set_err(FX_E_ARG, "bad out_mem %d", out_mem);
    if (!h) return set_err(FX_E_ARG, "null pq index");
    if (n == 0) return FX_OK;
    if (!out) return set_err(FX_E_ARG, "null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (i0 + n > h->ntotal)
        return set_err(FX_E_ARG, "pq reconstruct_n: rows [%lld, %lld) outside [0, %lld)", (long long)i0,
                       (long long)(i0 + n), (long long)h->ntotal);
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    float* od = out;
    if (out_mem == FX_MEM_HOST) {
        HIP_TRY(h->io.ensure((size_t)n * h->d * 4));
        od = (float*)h->io.p;
    }
    HIP_TRY(launch_pq_decode(h->codes, h->stride, h->ntotal, nullptr, i0, n, h->M, h->dsub, h->cb, od, s));
    if (out_mem == FX_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(out, od, (size_t)n * h->d * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return FX_OK;
}

int fx_pq_get_codes(FxPq* h, int64_t i0, int64_t n, uint8_t* out, int out_mem) {
    if (n < 0 || i0 < 0) return set_err(FX_E_ARG, "negative i0 / n");
    if (!valid_mem(out_mem)) return set_err(FX_E_ARG, "bad out_mem %d", out_mem);
    if (!h) return set_err(FX_E_ARG, "null pq index");
    if (n == 0) return FX_OK;
    if (!out) return set_err(FX_E_ARG, "null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (i0 + n > h->ntotal)
        return set_err(FX_E_ARG, "pq get_codes: rows [%lld, %lld) outside [0, %lld)", (long long)i0,
                       (long long)(i0 + n), (long long)h->ntotal);
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    // the rows' first M bytes, densely: faiss's [n][M]
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)h->M, h->codes + (size_t)i0 * h->stride, (size_t)h->stride, (size_t)h->M,
                             (size_t)n, out_mem == FX_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
    if (out_mem == FX_MEM_HOST) HIP_TRY(hipStreamSynchronize(s));
    return FX_OK;
}

int fx_pq_encode(FxPq* h, int64_t n, const void* x, int x_dtype, uint8_t* codes, int mem) {
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (!check_dtype(x_dtype)) return set_err(FX_E_ARG, "bad x dtype %d", x_dtype);
    if (!valid_mem(mem)) return set_err(FX_E_ARG, "bad mem %d", mem);
    if (!h) return set_err(FX_E_ARG, "null pq index");
    if (n == 0) return FX_OK;
    if (!x || !codes) return set_err(FX_E_ARG, "null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = pq_need_trained(h, "pq encode"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    const void* xd = nullptr;
    HIP_TRY(pq_stage_in(h, h->in, x, (size_t)n * h->d * dtype_size(x_dtype), mem, &xd));
    uint8_t* od = codes;
    if (mem == FX_MEM_HOST) {
        HIP_TRY(h->io.ensure((size_t)n * h->M));
        od = (uint8_t*)h->io.p;
    }
    HIP_TRY(launch_pq_encode(xd, x_dtype, n, h->d, h->M, h->dsub, h->cb, od, h->M, s));
    if (mem == FX_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(codes, od, (size_t)n * h->M, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return FX_OK;
}

int fx_pq_decode(FxPq* h, int64_t n, const uint8_t* codes, float* out, int mem) {
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (!valid_mem(mem)) return set_err(FX_E_ARG, "bad mem %d", mem);
    if (!h) return set_err(FX_E_ARG, "null pq index");
    if (n == 0) return FX_OK;
    if (!codes || !out) return set_err(FX_E_ARG, "null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = pq_need_trained(h, "pq decode"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    const void* cd = nullptr;
    HIP_TRY(pq_stage_in(h, h->in, codes, (size_t)n * h->M, mem, &cd));
    float* od = out;
    if (mem == FX_MEM_HOST) {
        HIP_TRY(h->io.ensure((size_t)n * h->d * 4));
        od = (float*)h->io.p;
    }
    HIP_TRY(launch_pq_decode((const uint8_t*)cd, h->M, n, nullptr, 0, n, h->M, h->dsub, h->cb, od, s));
    if (mem == FX_MEM_HOST) {
        HIP_TRY(hipMemcpyAsync(out, od, (size_t)n * h->d * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return FX_OK;
}

int fx_pq_set_stream(FxPq* h, void* stream) {
    if (!h) return set_err(FX_E_ARG, "null pq index");
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

int fx_pq_last_counts(FxPq* h, int64_t* fallbacks, int64_t* exact_fallbacks, int64_t* dropped) {
    if (!h || !fallbacks || !exact_fallbacks || !dropped) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = pq_read_counts(h); rc != FX_OK) return rc;
    *fallbacks = h->last_fallbacks;
    *exact_fallbacks = h->last_fallbacks;
    *dropped = h->last_dropped;
    return FX_OK;
}

int fx_pq_last_plan(FxPq* h, int* path, int* qtiles, int* splits, int* xsplits, int64_t* q_batch, int64_t* grid) {
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

int fx_pq_profile(FxPq* h, int enable) {
    if (!h) return set_err(FX_E_ARG, "null pq index");
    std::lock_guard<std::mutex> lk(h->mu);
    h->profile = enable != 0;
    return FX_OK;
}

int fx_pq_profile_read(FxPq* h, double* prep_ms, double* scan_ms, double* refine_ms, int64_t* passes) {
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

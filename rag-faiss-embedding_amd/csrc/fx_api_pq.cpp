// fx_api_pq.cpp -- product quantizer (fx_pq.hip): fx_pq_create / _set_centroids / _add / _search, the codec and
// the accessors.  The index owns its codes, row constants, centroids and their scan image; nothing of the flat
// index's state is shared.  Training is the caller's (M k-means runs, the Python layer): the centroids arrive
// through fx_pq_set_centroids, which rebuilds the scan image and the bound's constants on the host.
// The handle, the row store and the search driver are the shared ones (fx_host.h, fx_flat_codes.h).
#include "fx_flat_codes.h"

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

// fx_pq_search's part of flat_codes_search
struct PqOps {
    static SqPlan plan(const FxPq* h, int64_t nq, int k) { return plan_pq(nq, h->ntotal, k, h->M, h->dsub); }
    static hipError_t size(FxPq* h, int64_t, int64_t pad_max) {
        hipError_t e = h->qf32.ensure((size_t)pad_max * h->kp * 4);
        if (e == hipSuccess) e = h->planes.ensure((size_t)2 * pad_max * h->kp * 2);
        return e;
    }
    // fp32 copies, the [hi | lo] planes, the bound
    static hipError_t prep(FxPq* h, const CodePass& ps) {
        PqPrep pp{};
        pp.q = ps.q;
        pp.q_dt = ps.q_dt;
        pp.metric = h->metric;
        pp.d = h->d;
        pp.kp = h->kp;
        pp.nq = ps.nq;
        pp.nq_pad = ps.nq_pad;
        pp.Y = h->Y;
        pp.Ry = h->Ry;
        pp.Yl = h->Yl;
        pp.qf32 = (float*)h->qf32.p;
        pp.planes = (uint16_t*)h->planes.p;
        pp.qeps = (float*)h->eps.p;
        pp.qrho = (float*)h->rho.p;
        pp.qshift = (double*)h->shift.p;
        pp.zero[0] = ps.n_flag;
        pp.zero[1] = nullptr;
        return launch_pq_prep(pp, ps.s);
    }
    // the gather scan
    static hipError_t scan(FxPq* h, const CodePass& ps) {
        PqScan sc{};
        sc.codes = h->u8();
        sc.ny = h->nc;
        sc.ntotal = h->ntotal;
        sc.stride = h->stride;
        sc.M = h->M;
        sc.dsub = h->dsub;
        sc.d = h->d;
        sc.kp = h->kp;
        sc.img = h->img;
        sc.plane_bytes = pq_plane_bytes(h->M, h->dsub);
        sc.planes = (uint16_t*)h->planes.p;
        sc.nq = ps.nq;
        sc.nq_pad = ps.nq_pad;
        sc.n_qtiles = (int)(ps.nq_pad / TILE_Q);
        sc.n_ctiles = (int)((h->ntotal + TILE_R - 1) / TILE_R);
        sc.splits = ps.P->splits;
        sc.cand_d = (float*)h->cand_d.p;
        sc.cand_i = (int*)h->cand_i.p;
        return launch_pq_scan(h->metric, sc, ps.s);
    }
#ifdef FX_DIAG
    // FX_PQ_CAND: the pass's scan lists, query operands and the rows' constants appended to the file:
    //   cand_d, cand_i [qtiles][splits][128][KP] | qeps [nq] | qshift [nq] f64 |
    //   planes [2][nq_pad][kp] bf16 | codes [ntotal][stride] u8 | n_y [ntotal]
    static int dump(FxPq* h, const CodePass& ps) {
        const std::string& path = h->opt.pq_cand;
        if (path.empty()) return FX_OK;
        const size_t ncand = (size_t)(ps.nq_pad / TILE_Q) * ps.P->splits * TILE_Q * KP;
        HIP_TRY(hipStreamSynchronize(ps.s));
        HIP_TRY(dump_device<float>(path, h->cand_d.p, ncand));
        HIP_TRY(dump_device<int>(path, h->cand_i.p, ncand));
        HIP_TRY(dump_device<float>(path, h->eps.p, (size_t)ps.nq));
        HIP_TRY(dump_device<double>(path, h->shift.p, (size_t)ps.nq));
        HIP_TRY(dump_device<uint16_t>(path, h->planes.p, (size_t)2 * ps.nq_pad * h->kp));
        HIP_TRY(dump_device<uint8_t>(path, h->codes, (size_t)h->ntotal * h->stride));
        HIP_TRY(dump_device<float>(path, h->nc, (size_t)h->ntotal));
        return FX_OK;
    }
#endif
    static hipError_t refine(FxPq* h, const CodePass& ps) {
        PqRefine rp{};
        rp.cand_d = (float*)h->cand_d.p;
        rp.cand_i = (int*)h->cand_i.p;
        rp.splits = ps.P->splits;
        rp.nq = ps.nq;
        rp.ntotal = h->ntotal;
        rp.k = ps.k;
        rp.d = h->d;
        rp.kp = h->kp;
        rp.M = h->M;
        rp.dsub = h->dsub;
        rp.stride = h->stride;
        rp.codes = h->u8();
        rp.cb = h->cb;
        rp.qf32 = (float*)h->qf32.p;
        rp.qeps = (float*)h->eps.p;
        rp.qshift = (double*)h->shift.p;
        rp.D = ps.D;
        rp.I = ps.I;
        rp.n_flag = ps.n_flag;
        rp.n_drop = h->cnt;
        rp.force_fb = h->opt.force_fallback != 0;
        return launch_pq_refine(h->metric, rp, ps.s);
    }
    static hipError_t exact(FxPq* h, const CodePass& ps) {
        PqExact ex{};
        ex.codes = h->u8();
        ex.stride = h->stride;
        ex.M = h->M;
        ex.dsub = h->dsub;
        ex.d = h->d;
        ex.kp = h->kp;
        ex.ntotal = h->ntotal;
        ex.cb = h->cb;
        ex.qf32 = (float*)h->qf32.p;
        ex.n_flag = ps.n_flag;
        ex.k = ps.k;
        ex.xs = ps.P->xsplits;
        ex.cd = (float*)h->cand_d.p;
        ex.ci = (int*)h->cand_i.p;
        ex.D = ps.D;
        ex.I = ps.I;
        return launch_pq_exact(h->metric, ex, ps.s);
    }
};

}  // namespace

namespace fx {

int pq_codebook(const char* kind, int M, int dsub, const float* centroids, PqCodebook& out) {
    const size_t nval = (size_t)M * PQ_KSUB * dsub;
    for (size_t i = 0; i < nval; ++i)
        if (!std::isfinite(centroids[i]))
            return set_err(FX_E_ARG, "%s set_centroids: centroid %lld of sub-quantizer %lld has a non-finite value", kind,
                           (long long)(i / dsub % PQ_KSUB), (long long)(i / dsub / PQ_KSUB));
    // the bound's constants: per sub-quantizer maxima, so they hold for any code row; the scan image
    const bool scan = dsub % 8 == 0;
    const size_t plane = (size_t)pq_plane_bytes(M, dsub) / 2;  // bf16 values of a plane
    out.img.assign(scan ? 2 * plane : 0, 0);
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
                    out.img[i] = hb;
                    out.img[plane + i] = lb;
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
        return set_err(FX_E_ARG, "%s set_centroids: the centroids' norms leave the fp32 range", kind);
    const double up = 1.0 + 1e-9;
    out.Y = std::sqrt(y2) * up;
    out.Ry = std::sqrt(r2) * up;
    out.Yl = std::sqrt(l2) * up;
    return FX_OK;
}

}  // namespace fx

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
    hipError_t e = h->init();
    if (e == hipSuccess) e = h->cb.ensure((size_t)M * PQ_KSUB * h->dsub * 4);
    if (e == hipSuccess && h->dsub % 8 == 0) e = h->img.ensure((size_t)2 * pq_plane_bytes(M, h->dsub));
    if (e != hipSuccess) {
        fx_pq_free(h);
        return set_err(FX_E_HIP, "pq init: %s", hipGetErrorString(e));
    }
    *out = h;
    return FX_OK;
}

void fx_pq_free(FxPq* h) { handle_free(h); }

int fx_pq_is_trained(const FxPq* h, int* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    *out = h->trained ? 1 : 0;
    return FX_OK;
}

int fx_pq_get_centroids(FxPq* h, float* out) {
    if (!h || !out) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = need_trained(h->trained, "pq", "get_centroids"); rc != FX_OK) return rc;
    memcpy(out, h->h_cb.data(), h->h_cb.size() * 4);
    return FX_OK;
}

int fx_pq_set_centroids(FxPq* h, const float* centroids) {
    if (!h || !centroids) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->ntotal > 0)
        return set_err(FX_E_ARG, "pq set_centroids: the index holds %lld rows (reset it first)", (long long)h->ntotal);
    const size_t nval = (size_t)h->M * PQ_KSUB * h->dsub;
    PqCodebook cbk;
    if (const int rc = pq_codebook("pq", h->M, h->dsub, centroids, cbk); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    hipStream_t s = h->stream();
    HIP_TRY(hipStreamSynchronize(s));  // (an earlier search may still read the image)
    HIP_TRY(hipMemcpyAsync(h->cb, centroids, nval * 4, hipMemcpyHostToDevice, s));
    if (!cbk.img.empty()) HIP_TRY(hipMemcpyAsync(h->img, cbk.img.data(), cbk.img.size() * 2, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    h->h_cb.assign(centroids, centroids + nval);
    h->Y = cbk.Y;
    h->Ry = cbk.Ry;
    h->Yl = cbk.Yl;
    h->trained = true;
    return FX_OK;
}

int fx_pq_add(FxPq* h, int64_t n, const void* x, int x_dtype, int x_mem) {
    if (const int rc = check_rows(n, x_dtype, x_mem); rc != FX_OK) return rc;
    if (!h) return set_err(FX_E_ARG, "null pq index");
    if (n == 0) return FX_OK;
    if (!x) return set_err(FX_E_ARG, "null x");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = need_trained(h->trained, "pq", "add"); rc != FX_OK) return rc;
    if (h->ntotal + n + 2 * TILE_R >= (int64_t)INT32_MAX) return set_err(FX_E_UNSUPPORTED, "pq: more than 2^31-1 rows");
    DeviceGuard g(h->device);
    if (!g.ok) return set_err(FX_E_HIP, "hipSetDevice(%d) failed", h->device);
    hipStream_t s = h->stream();
    HIP_TRY(h->grow(h->ntotal + n, s));
    const int rc = staged_rows(s, h->in, n, x, (size_t)h->d * dtype_size(x_dtype), x_mem, 0,
                               [&](const void* xd, int64_t r0, int64_t nr) {
                                   uint8_t* c0 = h->u8() + (size_t)(h->ntotal + r0) * h->stride;
                                   HIP_TRY(launch_pq_encode(xd, x_dtype, nr, h->d, h->M, h->dsub, h->cb, c0, h->stride, s));
                                   HIP_TRY(launch_pq_ny(c0, h->stride, nr, h->M, h->dsub, h->cb, h->nc + h->ntotal + r0, s));
                                   return (int)FX_OK;
                               });
    if (rc == FX_OK) h->ntotal += n;
    return rc;
}

int fx_pq_search(FxPq* h, int64_t nq, const void* q, int q_dtype, int q_mem, int k, float* D, int64_t* I, int out_mem) {
    return flat_codes_search<PqOps>(h, "pq", nq, q, q_dtype, q_mem, k, D, I, out_mem);
}

int fx_pq_reset(FxPq* h) {
    if (!h) return set_err(FX_E_ARG, "null pq index");
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(h->zero(s));
    h->ntotal = 0;
    h->clear_counts();
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
    if (const int rc = need_trained(h->trained, "pq", "reconstruct"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    const size_t bytes = (size_t)n * h->d * 4;
    const void* kd = nullptr;
    void* od = nullptr;
    HIP_TRY(stage_in(s, h->in, keys, (size_t)n * 8, keys_mem, &kd));
    HIP_TRY(out_buf(h->io, out, bytes, out_mem, &od));
    HIP_TRY(launch_pq_decode(h->u8(), h->stride, h->ntotal, (const int64_t*)kd, 0, n, h->M, h->dsub, h->cb, (float*)od, s));
    return finish_out(s, out, od, bytes, out_mem, keys_mem == FX_MEM_HOST);
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
    const size_t bytes = (size_t)n * h->d * 4;
    void* od = nullptr;
    HIP_TRY(out_buf(h->io, out, bytes, out_mem, &od));
    HIP_TRY(launch_pq_decode(h->u8(), h->stride, h->ntotal, nullptr, i0, n, h->M, h->dsub, h->cb, (float*)od, s));
    return finish_out(s, out, od, bytes, out_mem);
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
    if (const int rc = need_trained(h->trained, "pq", "encode"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    const size_t bytes = (size_t)n * h->M;
    const void* xd = nullptr;
    void* od = nullptr;
    HIP_TRY(stage_in(s, h->in, x, (size_t)n * h->d * dtype_size(x_dtype), mem, &xd));
    HIP_TRY(out_buf(h->io, codes, bytes, mem, &od));
    HIP_TRY(launch_pq_encode(xd, x_dtype, n, h->d, h->M, h->dsub, h->cb, (uint8_t*)od, h->M, s));
    return finish_out(s, codes, od, bytes, mem);
}

int fx_pq_decode(FxPq* h, int64_t n, const uint8_t* codes, float* out, int mem) {
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (!valid_mem(mem)) return set_err(FX_E_ARG, "bad mem %d", mem);
    if (!h) return set_err(FX_E_ARG, "null pq index");
    if (n == 0) return FX_OK;
    if (!codes || !out) return set_err(FX_E_ARG, "null buffer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (const int rc = need_trained(h->trained, "pq", "decode"); rc != FX_OK) return rc;
    DeviceGuard g(h->device);
    hipStream_t s = h->stream();
    const size_t bytes = (size_t)n * h->d * 4;
    const void* cd = nullptr;
    void* od = nullptr;
    HIP_TRY(stage_in(s, h->in, codes, (size_t)n * h->M, mem, &cd));
    HIP_TRY(out_buf(h->io, out, bytes, mem, &od));
    HIP_TRY(launch_pq_decode((const uint8_t*)cd, h->M, n, nullptr, 0, n, h->M, h->dsub, h->cb, (float*)od, s));
    return finish_out(s, out, od, bytes, mem);
}

int fx_pq_set_stream(FxPq* h, void* stream) { return handle_set_stream(h, "pq", stream); }

int fx_pq_last_counts(FxPq* h, int64_t* fallbacks, int64_t* exact_fallbacks, int64_t* dropped) {
    return handle_last_counts(h, nullptr, fallbacks, exact_fallbacks, dropped);
}

int fx_pq_last_plan(FxPq* h, int* path, int* qtiles, int* splits, int* xsplits, int64_t* q_batch, int64_t* grid) {
    return flat_codes_last_plan(h, path, qtiles, splits, xsplits, q_batch, grid);
}

int fx_pq_profile(FxPq* h, int enable) { return handle_profile(h, "pq", enable); }

int fx_pq_profile_read(FxPq* h, double* prep_ms, double* scan_ms, double* refine_ms, int64_t* passes) {
    double* const ms[] = {prep_ms, scan_ms, refine_ms};
    return handle_profile_read(h, ms, passes);
}

}  // extern "C"

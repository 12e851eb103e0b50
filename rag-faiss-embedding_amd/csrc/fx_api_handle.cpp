// fx_api_handle.cpp -- what FxSq, FxPq, FxIvfSq and FxIvf share (fx_host.h): the handle core (stream,
// counts, profile), the code-row store, and the helpers of a call's input and output.
#include "fx_host.h"

namespace fx {

int fill_missing(hipStream_t s, int metric, int64_t nq, int k, float* D, int64_t* I, int out_mem) {
    const size_t n = (size_t)nq * k;
    std::vector<float> hd(n, metric == L2 ? FLT_MAX : -FLT_MAX);
    std::vector<int64_t> hi(n, -1);
    if (out_mem == FX_MEM_HOST) {
        memcpy(D, hd.data(), n * 4);
        memcpy(I, hi.data(), n * 8);
        return FX_OK;
    }
    HIP_TRY(hipMemcpyAsync(D, hd.data(), n * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(I, hi.data(), n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // (the host vectors go out of scope)
    return FX_OK;
}

hipError_t out_buf(DevBuf& io, void* out, size_t bytes, int out_mem, void** od) {
    *od = out;
    if (out_mem != FX_MEM_HOST) return hipSuccess;
    hipError_t e = io.ensure(bytes);
    *od = io.p;
    return e;
}

int finish_out(hipStream_t s, void* out, const void* od, size_t bytes, int out_mem, bool wait) {
    if (out_mem == FX_MEM_HOST) HIP_TRY(hipMemcpyAsync(out, od, bytes, hipMemcpyDeviceToHost, s));
    if (out_mem == FX_MEM_HOST || wait) HIP_TRY(hipStreamSynchronize(s));
    return FX_OK;
}

int need_trained(bool trained, const char* kind, const char* call) {
    if (!trained) return set_err(FX_E_ARG, "%s %s: the index is not trained", kind, call);
    return FX_OK;
}

int check_rows(int64_t n, int x_dtype, int x_mem) {
    if (n < 0) return set_err(FX_E_ARG, "negative n");
    if (!check_dtype(x_dtype)) return set_err(FX_E_ARG, "bad x dtype %d", x_dtype);
    if (!valid_mem(x_mem)) return set_err(FX_E_ARG, "bad x_mem %d", x_mem);
    return FX_OK;
}

int sq_check_tables(const char* kind, int d, const float* trained) {
    for (int j = 0; j < d; ++j)
        if (!std::isfinite(trained[j]) || !std::isfinite(trained[d + j]) || trained[d + j] < 0.f)
            return set_err(FX_E_ARG, "%s set_trained: dimension %d has vmin = %g, vdiff = %g", kind, j,
                           (double)trained[j], (double)trained[d + j]);
    return FX_OK;
}

hipError_t SearchStats::init_counts() {
    hipError_t e = cnt.ensure(16);
    if (e == hipSuccess) e = hipMemset(cnt, 0, 16);
    if (e == hipSuccess) e = pin_cnt.ensure(16);
    if (e == hipSuccess) pin_cnt[0] = pin_cnt[1] = pin_cnt[2] = 0;
    return e;
}

hipError_t SearchStats::begin_pass(hipEvent_t* pass_ev, int n, hipStream_t s) {
    if (!profile) return hipSuccess;
    for (int i = 0; i < n; ++i)
        if (hipError_t e = hipEventCreate(&pass_ev[i]); e != hipSuccess) return e;
    ev.insert(ev.end(), pass_ev, pass_ev + n);
    return hipEventRecord(pass_ev[0], s);
}

void SearchStats::destroy_events() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    ev.clear();
}

int SearchStats::read_counts(int device, hipStream_t s, FxIndex* quant) {
    if (!counts_pending) return FX_OK;
    DeviceGuard g(device);
    HIP_TRY(hipStreamSynchronize(s));
    last_dropped = pin_cnt[0];
    last_fallbacks = pin_cnt[1];
    if (quant) last_bad_probe = pin_cnt[2];
    counts_pending = false;
    if (!quant) return FX_OK;
    // the borrowed coarse search's own integrity count (of the last pass; its copies ran on this stream)
    std::lock_guard<std::mutex> ql(quant->mu);
    return fx::read_counts(quant);
}

int SearchStats::profile_read(int device, hipStream_t s, int per_pass, double* const* ms, int64_t* passes) {
    if (!passes) return set_err(FX_E_ARG, "null argument");
    for (int part = 0; part + 1 < per_pass; ++part)
        if (!ms[part]) return set_err(FX_E_ARG, "null argument");
    DeviceGuard g(device);
    HIP_TRY(hipStreamSynchronize(s));
    double sum[4] = {0, 0, 0, 0};
    float t = 0;
    for (size_t i = 0; i + per_pass <= ev.size(); i += per_pass)
        for (int part = 0; part + 1 < per_pass; ++part) {
            HIP_TRY(hipEventElapsedTime(&t, ev[i + part], ev[i + part + 1]));
            sum[part] += t;
        }
    *passes = (int64_t)(ev.size() / per_pass);
    destroy_events();
    for (int part = 0; part + 1 < per_pass; ++part) *ms[part] = sum[part];
    return FX_OK;
}

hipError_t Handle::init() {
    opt.from_env();
    hipError_t e = hipStreamCreateWithFlags(&own_stream, hipStreamDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&switch_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = init_counts();
    return e;
}

int handle_set_stream(Handle* h, const char* kind, void* stream) {
    if (!h) return set_err(FX_E_ARG, "null %s index", kind);
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

hipError_t CodeRows::grow(int64_t n, hipStream_t s) {
    const int64_t want = round_up(n, TILE_R) + TILE_R;
    if (want <= cap_rows) return hipSuccess;
    const int64_t cap = std::max(want, round_up(cap_rows + cap_rows / 2, TILE_R));
    const size_t n0 = (size_t)ntotal;
    DevBuf c2, nc2, lab2, rl2;
    hipError_t e = c2.ensure((size_t)cap * stride);
    if (e == hipSuccess) e = nc2.ensure((size_t)cap * 4);
    if (e == hipSuccess && lists) e = lab2.ensure((size_t)cap * 8);
    if (e == hipSuccess && lists) e = rl2.ensure((size_t)cap * 4);
    if (e == hipSuccess) e = hipMemsetAsync(c2.p, 0, (size_t)cap * stride, s);
    if (e == hipSuccess) e = hipMemsetAsync(nc2.p, 0, (size_t)cap * 4, s);
    if (e == hipSuccess && n0 > 0) e = hipMemcpyAsync(c2.p, codes.p, n0 * stride, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && n0 > 0) e = hipMemcpyAsync(nc2.p, nc.p, n0 * 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && n0 > 0 && lists) e = hipMemcpyAsync(lab2.p, labels.p, n0 * 8, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && n0 > 0 && lists) e = hipMemcpyAsync(rl2.p, row_list.p, n0 * 4, hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // (work in flight still reads the old buffers)
    if (e != hipSuccess) return e;
    codes.swap(c2);
    nc.swap(nc2);
    labels.swap(lab2);
    row_list.swap(rl2);
    cap_rows = cap;
    return hipSuccess;
}

hipError_t CodeRows::zero(hipStream_t s) {
    if (cap_rows == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(codes, 0, (size_t)cap_rows * stride, s);
    if (e == hipSuccess) e = hipMemsetAsync(nc, 0, (size_t)cap_rows * 4, s);
    return e;
}

}  // namespace fx

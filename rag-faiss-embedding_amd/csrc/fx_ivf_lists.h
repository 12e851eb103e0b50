// fx_ivf_lists.h -- what the inverted files (FxIvf, FxIvfSq, FxIvfPq) share beyond the handle core: the regroup
// into list order, the rules of an add, the coarse / pairs steps and the ends of a search, the list
// accessors (fx_api_ivf.cpp defines them).  The list scan, refine and exact steps are each file's own.
#pragma once
#include "fx_plan.h"

namespace fx {

// the payload arrays a regroup permutes: n rows of row_bytes, their constants, labels and lists
struct IvfRows {
    int64_t n, cap_rows;
    int row_bytes;
    DevBuf &codes, &norms, &labels, &row_list;
};
// The payload in list order (a no-op unless rows were added since): a stable sort of list << 32 | row
// keys and a gather into second buffers, swapped in and released again.  zero_incoming: the second
// codes / constants start as zeros (rows past n must hold code 0 and constant 0).  `bad`: the device
// count of assignments outside the lists since the last read.
int ivf_regroup(const char* kind, IvfLists& L, const IvfRows& R, bool zero_incoming, unsigned long long* bad,
                hipStream_t s);
int ivf_bad_error(const char* kind, int64_t bad, int64_t nlist);
// the skipped-assignment count since the last read, then 0 again (synchronises)
int ivf_read_bad(unsigned long long* bad, hipStream_t s, int64_t* out);
// "<who>: the index is not trained (the quantizer holds ...)"
int ivf_quant_trained(const IvfLists& L, const char* who);
// an index holds sequential ids or labels, as its first add decided
int ivf_add_mode(const IvfLists& L, int64_t ntotal, const int64_t* ids);

// a search's argument checks (the handle's own check comes after them), and its probe count
int ivf_search_args(const char* kind, int64_t nq, int k, int nprobe, int q_dtype, int q_mem, int out_mem);
int ivf_probes(const char* kind, const IvfLists& L, int64_t nq, int nprobe, int* np);
// the plan's record, and the workspace of the coarse search, the candidate lists and (fused) the pairs
hipError_t ivf_search_workspace(IvfLists& L, const IvfPlan& P, int64_t nq, int np, int k);
// the quantizer's exact top-np search of a pass, on stream s: coarse_d / coarse_i
int ivf_coarse(IvfLists& L, hipStream_t s, int64_t qb, const void* q, int q_dtype, int np);
// the pass's (query, list) pairs grouped by list: psorted, seg, gbase; bad_cnt counts entries outside the lists
hipError_t ivf_pairs(IvfLists& L, int* bad_cnt, int64_t qb, int np, hipStream_t s);
// the counts' copy, a host caller's results and the integrity error
int ivf_search_finish(const char* kind, SearchStats& st, const IvfLists& L, int device, hipStream_t s, int64_t nq, int k,
                      float* D, const void* Dd, int64_t* I, const void* Id, int out_mem, int64_t ntotal);

// the accessors of a handle type V (FxIvf, FxIvfSq); regroup(v) brings its payload into list order
template <class V, class Regroup>
int ivf_list_sizes(V* v, Regroup regroup, int64_t* out) {
    if (!v || !out) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(v->mu);
    DeviceGuard g(v->device);
    if (const int rc = regroup(v); rc != FX_OK) return rc;
    for (int64_t l = 0; l < v->nlist; ++l) out[l] = (int64_t)v->h_off[l + 1] - v->h_off[l];
    return FX_OK;
}
template <class V, class Regroup>
int ivf_list_ids(V* v, const char* kind, Regroup regroup, const DevArr<int64_t>& labels, int64_t list, int64_t* out,
                 int64_t cap, int64_t* n) {
    if (!v || !n) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(v->mu);
    if (list < 0 || list >= v->nlist)
        return set_err(FX_E_ARG, "%s list_ids: list %lld outside [0, %lld)", kind, (long long)list, (long long)v->nlist);
    DeviceGuard g(v->device);
    if (const int rc = regroup(v); rc != FX_OK) return rc;
    const int64_t r0 = v->h_off[list], cnt = (int64_t)v->h_off[list + 1] - r0;
    *n = cnt;
    if (cnt == 0 || cap <= 0) return FX_OK;
    if (!out) return set_err(FX_E_ARG, "null buffer");
    return finish_out(v->stream(), out, labels + r0, (size_t)std::min(cnt, cap) * 8, FX_MEM_HOST);
}
template <class V>
int ivf_last_plan(V* v, int* path, int* chunks, int* slots, int64_t* q_batch, int64_t* grid) {
    if (!v || !path || !chunks || !slots || !q_batch || !grid) return set_err(FX_E_ARG, "null argument");
    std::lock_guard<std::mutex> lk(v->mu);
    *path = v->last_plan[0];
    *chunks = v->last_plan[1];
    *slots = v->last_plan[2];
    *q_batch = v->last_qbatch;
    *grid = v->last_grid;
    return FX_OK;
}

}  // namespace fx

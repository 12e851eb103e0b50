// fx_recon.hip -- stored vectors and exact distances by key, on the device:
// faiss's reconstruct_batch / search_and_reconstruct / compute_distance_subset
// on the flat index.
//
//   k_gather_rows<DT, OUT32, VEC, G>   out[i][0..d) <- the stored row keys[i]
//                (fp32: exact widening of bf16 / fp16; or the storage dtype: a
//                byte copy of the d elements).  G lanes per row read 16 B each:
//                a whole wave for rows of more than 16 chunks (the key is then
//                wave-uniform), a 16-lane group per row for shorter ones.  The
//                stored rows are row_bytes-strided and zero-padded past d; `out`
//                is dense [n][d], so a chunk's elements at or past d are never
//                written.
//   k_subset_dist<DT, METRIC>          D[i][j] <- the exact distance of query i
//                and row keys[i][j]: exact_partial over 16 lanes per pair and
//                the refine's xor reduction, so the value is the one search
//                returns for that pair on the certified path.
//   k_label_ids                        I[i] <- labels[I[i]] (search_and_reconstruct
//                on a labelled index: the search ranks and the gather reads ROWS,
//                labels may repeat; I is translated last).
//
// The bounds rule: every key is checked against [id_offset, id_offset + ntotal)
// BEFORE a row address is formed.  A key outside (-1, the "missing slot" of a
// search result, included) reads no memory and yields faiss's memset(-1) row
// of NaN (fp32 0xFFFFFFFF, 16-bit 0xFFFF) from the gather, and the library's
// missing-slot distance (L2: FLT_MAX, IP: -FLT_MAX) from the distance kernel.
//
// No LDS, no atomics; plain vector stores.  Grid-stride with the capped grid of
// the row kernels (ROWS_GRID_CAP, the finding recorded in fx_kernels.hip).
#include "fx_device.h"

namespace fx {

constexpr int RC_THREADS = 256;
constexpr int RC_GRID_CAP = 4096;  // == ROWS_GRID_CAP (fx_kernels.hip)

namespace {

unsigned rc_grid(int64_t waves) {
    const int64_t g = (waves + 3) / 4;  // 4 waves per workgroup
    return (unsigned)(g < 1 ? 1 : g > RC_GRID_CAP ? RC_GRID_CAP : g);
}

}  // namespace

// the local row of `key`, or -1 when the key names no row of the index
__device__ __forceinline__ int64_t rc_row_of(int64_t key, int64_t id_offset, int64_t ntotal) {
    // (id_offset >= 0: key - id_offset cannot overflow once key >= id_offset)
    if (key < id_offset) return -1;
    const int64_t row = key - id_offset;
    return row < ntotal ? row : (int64_t)-1;
}

__device__ __forceinline__ int64_t rc_uniform(int64_t v) {
    const int lo = __builtin_amdgcn_readfirstlane((int)(v & 0xffffffffll));
    const int hi = __builtin_amdgcn_readfirstlane((int)(v >> 32));
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}

// keys null: the implicit key key0 + i (reconstruct_n's contiguous rows)
template <int DT, bool OUT32, bool VEC, int G>
__global__ __launch_bounds__(RC_THREADS) void k_gather_rows(const char* __restrict__ codes, int row_bytes,
                                                            int64_t ntotal, const int64_t* __restrict__ keys,
                                                            int64_t key0, int64_t id_offset, int64_t n, int d,
                                                            void* __restrict__ out) {
    constexpr int E = DT == F32 ? 4 : 8;  // elements per 16-B chunk of a stored row
    constexpr int R = 64 / G;             // rows per wave pass
    const int lane = threadIdx.x & 63, sub = lane % G, grp = lane / G;
    const int nc = (d + E - 1) / E;       // chunks that hold an element below d
    const int64_t wave = (int64_t)blockIdx.x * (RC_THREADS / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (RC_THREADS / 64);
    for (int64_t i0 = wave * R; i0 < n; i0 += nwaves * R) {
        const int64_t i = i0 + grp;
        if (i >= n) continue;
        int64_t key = keys ? keys[i] : key0 + i;
        if constexpr (G == 64) key = rc_uniform(key);
        const int64_t row = rc_row_of(key, id_offset, ntotal);
        for (int c = sub; c < nc; c += G) {
            uint4 v = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
            if (row >= 0) v = *(const uint4*)(codes + row * row_bytes + (int64_t)c * 16);
            const int e0 = c * E;
            if constexpr (!OUT32 || DT == F32) {
                // the chunk's bytes as they are: E elements of the storage dtype
                char* o = (char*)out + (i * d + e0) * (int64_t)(DT == F32 ? 4 : 2);
                if constexpr (VEC) {  // d % E == 0: the chunk lies wholly below d
                    *(uint4*)o = v;
                } else if constexpr (DT == F32) {
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (e0 + e < d) ((uint32_t*)o)[e] = w[e];
                } else {
                    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (e0 + e < d) ((uint16_t*)o)[e] = (uint16_t)(w[e >> 1] >> ((e & 1) * 16));
                }
            } else {
                // 8 stored 16-bit elements -> 8 fp32 (exact); a NaN row stays all ones
                uint32_t f[8];
                const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const uint16_t h = (uint16_t)(w[e >> 1] >> ((e & 1) * 16));
                    f[e] = row >= 0 ? __float_as_uint(DT == BF16 ? bf2f(h) : h2f(h)) : 0xffffffffu;
                }
                uint32_t* o = (uint32_t*)out + (i * d + e0);
                if constexpr (VEC) {  // d % 4 == 0: each half lies wholly below d or wholly past it
                    *(uint4*)o = make_uint4(f[0], f[1], f[2], f[3]);
                    if (e0 + 4 < d) *(uint4*)(o + 4) = make_uint4(f[4], f[5], f[6], f[7]);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (e0 + e < d) o[e] = f[e];
                }
            }
        }
    }
}

template <int DT, int METRIC>
__global__ __launch_bounds__(RC_THREADS) void k_subset_dist(const char* __restrict__ codes, int row_bytes, int kdim,
                                                            int64_t ntotal, const float* __restrict__ qf32,
                                                            int64_t nq, int k, const int64_t* __restrict__ keys,
                                                            int64_t id_offset, float* __restrict__ D) {
    const int lane = threadIdx.x & 63, sub = lane & 15, grp = lane >> 4;
    const int64_t total = nq * k;
    const int64_t wave = (int64_t)blockIdx.x * (RC_THREADS / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (RC_THREADS / 64);
    for (int64_t p0 = wave * 4; p0 < total; p0 += nwaves * 4) {  // (wave-uniform: every lane joins the shuffles)
        const int64_t p = p0 + grp;
        const bool live = p < total;
        const int64_t row = live ? rc_row_of(keys[p], id_offset, ntotal) : (int64_t)-1;
        double a = 0.0;
        if (row >= 0)
            a = exact_partial<DT, METRIC>(qf32 + (p / k) * kdim, codes + row * row_bytes, row_bytes, sub, 16);
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        if (live && sub == 0) D[p] = row >= 0 ? (float)a : (METRIC == L2 ? FLT_MAX : -FLT_MAX);
    }
}

// I[i] (a row, or -1) -> the row's label
__global__ __launch_bounds__(RC_THREADS) void k_label_ids(const int64_t* __restrict__ labels, int64_t ntotal,
                                                          int64_t n, int64_t* __restrict__ I) {
    for (int64_t i = (int64_t)blockIdx.x * RC_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * RC_THREADS) {
        const int64_t row = I[i];
        I[i] = row >= 0 && row < ntotal ? labels[row] : (int64_t)-1;
    }
}

namespace {

template <int DT, bool OUT32>
hipError_t gather_launch(const char* codes, int row_bytes, int64_t ntotal, const int64_t* keys, int64_t key0,
                         int64_t id_offset, int64_t n, int d, void* out, hipStream_t s) {
    constexpr int E = DT == F32 ? 4 : 8;
    const int nc = (d + E - 1) / E;
    // whole 16-B stores: the output rows keep the vector's alignment and no vector straddles d
    const int oes = OUT32 ? 4 : (DT == F32 ? 4 : 2);
    const int per_store = 16 / oes;
    const bool vec = d % per_store == 0 && ((uintptr_t)out & 15) == 0;
    const bool wide = nc > 16;
    const unsigned grid = rc_grid(wide ? n : (n + 3) / 4);
#define FX_GATHER(V, GL)                                                                                         \
    hipLaunchKernelGGL((k_gather_rows<DT, OUT32, V, GL>), dim3(grid), dim3(RC_THREADS), 0, s, codes, row_bytes, \
                       ntotal, keys, key0, id_offset, n, d, out)
    if (vec && wide) FX_GATHER(true, 64);
    else if (vec) FX_GATHER(true, 16);
    else if (wide) FX_GATHER(false, 64);
    else FX_GATHER(false, 16);
#undef FX_GATHER
    return hipGetLastError();
}

}  // namespace

hipError_t launch_gather_rows(const char* codes, int st_dt, int row_bytes, int64_t ntotal, const int64_t* keys,
                              int64_t key0, int64_t id_offset, int64_t n, int d, void* out, int out_dt,
                              hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!out || d <= 0 || (out_dt != F32 && out_dt != st_dt) || (ntotal > 0 && !codes)) return hipErrorInvalidValue;
    return dispatch_dt_metric<DT_STORED>(st_dt, L2, [&](auto dtc, auto) {
        constexpr int DT = decltype(dtc)::value;
        if (out_dt == F32)
            return gather_launch<DT, true>(codes, row_bytes, ntotal, keys, key0, id_offset, n, d, out, s);
        return gather_launch<DT, false>(codes, row_bytes, ntotal, keys, key0, id_offset, n, d, out, s);
    });
}

hipError_t launch_subset_dist(int st_dt, int metric, const char* codes, int row_bytes, int kdim, int64_t ntotal,
                              const float* qf32, int64_t nq, int k, const int64_t* keys, int64_t id_offset, float* D,
                              hipStream_t s) {
    if (nq <= 0 || k <= 0) return hipSuccess;
    if (!qf32 || !keys || !D || (ntotal > 0 && !codes)) return hipErrorInvalidValue;
    const unsigned grid = rc_grid((nq * k + 3) / 4);
    return dispatch_dt_metric<DT_STORED>(st_dt, metric, [&](auto dtc, auto mc) {
        hipLaunchKernelGGL((k_subset_dist<decltype(dtc)::value, decltype(mc)::value>), dim3(grid), dim3(RC_THREADS), 0,
                           s, codes, row_bytes, kdim, ntotal, qf32, nq, k, keys, id_offset, D);
        return hipGetLastError();
    });
}

hipError_t launch_label_ids(const int64_t* labels, int64_t ntotal, int64_t n, int64_t* I, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!labels || !I) return hipErrorInvalidValue;
    const int64_t g = (n + RC_THREADS - 1) / RC_THREADS;
    hipLaunchKernelGGL(k_label_ids, dim3((unsigned)(g > RC_GRID_CAP ? RC_GRID_CAP : g)), dim3(RC_THREADS), 0, s, labels,
                       ntotal, n, I);
    return hipGetLastError();
}

}  // namespace fx

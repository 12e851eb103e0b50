// fx_kmeans.hip -- the update half of Lloyd's algorithm on the device: faiss's
// Clustering::train / faiss.Kmeans, given the assignment that a k = 1 search
// over the centroid index returns (the other half: fx_api_kmeans.cpp fx_kmeans_step).
//
// Everything here is bitwise reproducible: the result depends only on
// (x, assign, KM_M) and the order of the chunks, never on timing.  No floating
// point atomics, no workgroup waits on another; sums are fp64.
//
//   k_km_keys      key[i] = (uint64)assign[i] << 32 | i.  An assign[i] outside
//                  [0, k) -- a padded search's -1 included -- forms the key of
//                  the extra segment k (never summed) and is counted in `bad`
//                  (an integer atomic; the host fails the call on a non-zero
//                  count).
//   (hipCUB)       DeviceRadixSort::SortKeys over the bits of the cluster only,
//                  [32, 32 + bit_width(k)): the sort is stable and the keys are
//                  built in row order, so every cluster's members stay in
//                  ascending row order.
//   k_km_seg       seg[c] = first sorted position of cluster c (a binary search
//                  per cluster; seg[k] = the valid entries), nblk[c] = member
//                  blocks of KM_M rows; (hipCUB) DeviceScan::ExclusiveSum ->
//                  blk0[k + 1].
//   k_km_sum       one workgroup per (cluster, block of KM_M consecutive
//                  members).  Lanes own 16-B column slices of a row (the layout
//                  of k_gather_rows): a row of nc slices is read by nc lanes,
//                  and the workgroup's R = 256 / nc lane groups ("slots") read
//                  R rows at a time, 4 rows in flight per lane.  Each lane
//                  widens exactly and adds into fp64 registers in member order;
//                  the slots are then combined through LDS in slot order and
//                  the block's fp64 partial row is written.  A row index is
//                  checked against n before an address is formed; rows are
//                  dense [n][d] (no padding), so a slice past d is never read:
//                  rows whose bytes are not a multiple of 16, or a base that is
//                  not 16-B aligned, take element loads masked at d.
//   k_km_obj       per 4,096 rows, the fp64 sum of the valid rows' distances in
//                  a fixed tree.
//   k_km_fold      sums[c] (+)= the cluster's partial rows in ascending block
//                  order, counts[c] (+)= seg[c + 1] - seg[c]; its last workgroup
//                  adds the k_km_obj partials in a fixed tree into obj.
//
//   k_km_mean      centroid = (float)(sums / counts) where counts > 0; an empty
//                  cluster keeps the row the centroid index stores.
//   k_km_finish    empty-cluster repair, serial over the empty clusters inside
//                  one workgroup.  It follows faiss's split_clusters except for
//                  the donor: faiss draws it at random in proportion to the
//                  cluster sizes, this kernel takes the cluster with the
//                  largest working count (ties: the smaller index), so a
//                  training is reproducible.  For each empty ci in ascending
//                  order: c[ci] = c[cj]; even j: c[ci][j] *= 1 + EPS, c[cj][j]
//                  *= 1 - EPS, odd j the signs swapped (EPS = 1/1024);
//                  h[ci] = h[cj] / 2, h[cj] -= h[ci].
//   k_km_normalize spherical: every centroid divided by its L2 norm (an fp64
//                  sum in a fixed order; each element rounded once).
#include "fx_device.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace fx {

namespace {

constexpr int KM_THREADS = 256;
constexpr int KM_GRID_CAP = 4096;
constexpr int64_t KM_SUM_GRID_CAP = 1 << 20;  // k_km_sum strides over the member blocks past it
constexpr int KM_FIN_THREADS = 1024;
constexpr int KM_SORT_BEGIN = 32;  // the keys are sorted by their cluster bits only (a stable sort)
constexpr int KM_OBJ_ROWS = 4096;  // rows per k_km_obj workgroup

inline size_t km_align(size_t v) { return (v + 255) / 256 * 256; }

// bits that hold a cluster number 0 .. k (k: the segment of the invalid entries)
inline int km_bits(int64_t k) {
    int b = 1;
    while (((int64_t)1 << b) <= k) ++b;
    return b;
}

unsigned km_grid(int64_t items, int per_block) {
    const int64_t g = (items + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : g > KM_GRID_CAP ? KM_GRID_CAP : g);
}

struct KmCarve {
    size_t keys, sorted, seg, nblk, blk0, objp, partial, temp, temp_bytes, total;
    int64_t max_blocks;
    int obj_blocks;
};

hipError_t km_carve(int64_t n, int64_t k, int d, KmCarve* c) {
    size_t sort_tb = 0, scan_tb = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortKeys(nullptr, sort_tb, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                                     (int)n, KM_SORT_BEGIN, 32 + km_bits(k));
    if (e != hipSuccess) return e;
    e = hipcub::DeviceScan::ExclusiveSum(nullptr, scan_tb, (const int*)nullptr, (int*)nullptr, (int)(k + 1));
    if (e != hipSuccess) return e;
    // >= the sum over the non-empty clusters (at most min(n, k)) of ceil(members / KM_M)
    c->max_blocks = (n + KM_M - 1) / KM_M + std::min(n, k);
    c->obj_blocks = (int)((n + KM_OBJ_ROWS - 1) / KM_OBJ_ROWS);
    size_t o = 0;
    c->keys = o, o += km_align((size_t)n * 8);
    c->sorted = o, o += km_align((size_t)n * 8);
    c->seg = o, o += km_align((size_t)(k + 1) * 4);
    c->nblk = o, o += km_align((size_t)(k + 1) * 4);
    c->blk0 = o, o += km_align((size_t)(k + 1) * 4);
    c->objp = o, o += km_align((size_t)c->obj_blocks * 8);
    c->partial = o, o += km_align((size_t)c->max_blocks * d * 8);
    c->temp = o, c->temp_bytes = std::max(sort_tb, scan_tb), o += km_align(c->temp_bytes);
    c->total = o;
    return hipSuccess;
}

}  // namespace

__global__ __launch_bounds__(KM_THREADS) void k_km_keys(const int64_t* __restrict__ assign, int64_t n, int64_t k,
                                                        uint64_t* __restrict__ keys,
                                                        unsigned long long* __restrict__ bad) {
    for (int64_t i = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * KM_THREADS) {
        const int64_t a = assign[i];
        const bool ok = a >= 0 && a < k;
        keys[i] = (uint64_t)(ok ? a : k) << 32 | (uint32_t)i;
        if (!ok) atomicAdd(bad, 1ull);
    }
}

// first position of `sorted` whose cluster is >= c
__device__ __forceinline__ int km_lower(const uint64_t* __restrict__ sorted, int n, int64_t c) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((int64_t)(sorted[mid] >> 32) < c) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(KM_THREADS) void k_km_seg(const uint64_t* __restrict__ sorted, int n, int64_t k,
                                                       int* __restrict__ seg, int* __restrict__ nblk) {
    for (int64_t c = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x; c <= k; c += (int64_t)gridDim.x * KM_THREADS) {
        const int s0 = km_lower(sorted, n, c);
        seg[c] = s0;
        nblk[c] = c < k ? (km_lower(sorted, n, c + 1) - s0 + KM_M - 1) / KM_M : 0;
    }
}

// E elements of row `row` from column e0 on, widened exactly (0 past d)
template <int DT, bool VEC>
__device__ __forceinline__ void km_load(const char* __restrict__ x, int64_t row, int d, int e0, float* v) {
    constexpr int E = DT == F32 ? 4 : 8;
    if constexpr (VEC) {
        load_chunk<DT>(x + (row * d + e0) * (int64_t)(DT == F32 ? 4 : 2), v);
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) v[e] = e0 + e < d ? load_elem(x, row * d + e0 + e, DT) : 0.0f;
    }
}

template <int DT, bool VEC>
__global__ __launch_bounds__(KM_THREADS) void k_km_sum(const char* __restrict__ x, int64_t n, int d,
                                                       const uint64_t* __restrict__ sorted,
                                                       const int* __restrict__ seg, const int* __restrict__ blk0,
                                                       int64_t k, double* __restrict__ partial) {
    constexpr int E = DT == F32 ? 4 : 8;  // elements per 16-B slice
    constexpr int U = 4;                  // rows in flight per lane
    // [element][thread], rows of KM_RS doubles: lanes store consecutive doubles, and the
    // combine's lanes (element fastest) read KM_RS * e + slice: distinct banks for E = 8
    constexpr int KM_RS = KM_THREADS + 4;
    __shared__ double red[8 * KM_RS];
    const int t = threadIdx.x;
    const int nc = (d + E - 1) / E;  // slices of a row
    const int total = blk0[k];       // member blocks of this call (the grid is an upper bound)
    for (int b = blockIdx.x; b < total; b += gridDim.x) {
        // the cluster of block b: the last c with blk0[c] <= b (blk0[k] > b, so it has members)
        int64_t lo = 0, hi = k;
        while (hi - lo > 1) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (blk0[mid] <= b) lo = mid;
            else hi = mid;
        }
        const int m0 = seg[lo] + (b - blk0[lo]) * KM_M;
        const int m1 = min(m0 + KM_M, seg[lo + 1]);
        for (int c0 = 0; c0 < nc; c0 += KM_THREADS) {
            const int ncl = min(KM_THREADS, nc - c0);
            const int R = KM_THREADS / ncl;  // rows read side by side
            const int slot = t / ncl, e0 = (c0 + t - slot * ncl) * E;
            if (slot < R) {
                double acc[E];
#pragma unroll
                for (int e = 0; e < E; ++e) acc[e] = 0.0;
                for (int j = m0 + slot; j < m1; j += R * U) {
                    float v[U][E];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int ju = j + u * R;
                        // the row of member ju; one outside [0, n) forms no address
                        const int64_t row = ju < m1 ? (int64_t)(uint32_t)sorted[ju] : (int64_t)-1;
                        if (row >= 0 && row < n) {
                            km_load<DT, VEC>(x, row, d, e0, v[u]);
                        } else {
#pragma unroll
                            for (int e = 0; e < E; ++e) v[u][e] = 0.0f;
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int e = 0; e < E; ++e) acc[e] += (double)v[u][e];
                }
#pragma unroll
                for (int e = 0; e < E; ++e) red[e * KM_RS + t] = acc[e];
            }
            __syncthreads();
            // the slots added in slot order; lanes write consecutive columns
            for (int q = t; q < ncl * E; q += KM_THREADS) {
                const int cc = q / E, e = q % E;
                double s = red[e * KM_RS + cc];
                for (int r = 1; r < R; ++r) s += red[e * KM_RS + r * ncl + cc];
                const int col = c0 * E + q;
                if (col < d) partial[(int64_t)b * d + col] = s;
            }
            __syncthreads();
        }
    }
}

// 256 values, one per thread -> their sum in a fixed tree (every thread gets it)
__device__ __forceinline__ double km_block_sum(double v, double* red) {
    const int t = threadIdx.x;
    red[t] = v;
    for (int o = KM_THREADS / 2; o > 0; o >>= 1) {
        __syncthreads();
        if (t < o) red[t] += red[t + o];
    }
    __syncthreads();
    const double s = red[0];
    __syncthreads();
    return s;
}

__global__ __launch_bounds__(KM_THREADS) void k_km_obj(const float* __restrict__ dist,
                                                       const int64_t* __restrict__ assign, int64_t n, int64_t k,
                                                       double* __restrict__ objp) {
    __shared__ double red[KM_THREADS];
    double s = 0.0;
    const int64_t i0 = (int64_t)blockIdx.x * KM_OBJ_ROWS + threadIdx.x;
    for (int q = 0; q < KM_OBJ_ROWS / KM_THREADS; ++q) {
        const int64_t i = i0 + (int64_t)q * KM_THREADS;
        if (i < n) {
            const int64_t a = assign[i];
            if (a >= 0 && a < k) s += (double)dist[i];
        }
    }
    s = km_block_sum(s, red);
    if (threadIdx.x == 0) objp[blockIdx.x] = s;
}

// workgroups [0, gridDim.x - 1): the fold; the last one: obj
__global__ __launch_bounds__(KM_THREADS) void k_km_fold(const double* __restrict__ partial,
                                                        const int* __restrict__ seg, const int* __restrict__ blk0,
                                                        int64_t k, int d, double* __restrict__ sums,
                                                        int64_t* __restrict__ counts, const double* __restrict__ objp,
                                                        int obj_blocks, double* __restrict__ obj, int accumulate) {
    __shared__ double red[KM_THREADS];
    const int t = threadIdx.x;
    if (blockIdx.x == gridDim.x - 1) {
        double s = 0.0;
        for (int i = t; i < obj_blocks; i += KM_THREADS) s += objp[i];
        s = km_block_sum(s, red);
        if (t == 0) *obj = accumulate ? *obj + s : s;
        return;
    }
    const int dtiles = (d + KM_THREADS - 1) / KM_THREADS;
    const int64_t items = k * dtiles;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x - 1) {
        const int64_t c = it / dtiles;
        const int col = (int)(it - c * dtiles) * KM_THREADS + t;
        if (col < d) {
            double s = 0.0;
            for (int b = blk0[c]; b < blk0[c + 1]; ++b) s += partial[(int64_t)b * d + col];
            const int64_t o = c * d + col;
            sums[o] = accumulate ? sums[o] + s : s;
        }
        if (col == 0) {
            const int64_t m = seg[c + 1] - seg[c];
            counts[c] = accumulate ? counts[c] + m : m;
        }
    }
}

__global__ __launch_bounds__(KM_THREADS) void k_km_mean(const double* __restrict__ sums,
                                                        const int64_t* __restrict__ counts, int64_t k, int d,
                                                        const char* __restrict__ codes, int st_dt, int row_bytes,
                                                        float* __restrict__ cent, int64_t* __restrict__ h) {
    const int64_t total = k * d;
    for (int64_t i = (int64_t)blockIdx.x * KM_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * KM_THREADS) {
        const int64_t c = i / d;
        const int j = (int)(i - c * d);
        const int64_t m = counts[c];
        cent[i] = m > 0 ? (float)(sums[i] / (double)m) : load_elem(codes + c * row_bytes, j, st_dt);
        if (j == 0) h[c] = m > 0 ? m : 0;
    }
}

// Thread t owns the working counts h[c] and the columns j with c, j = t mod
// KM_FIN_THREADS: it alone reads and writes them, so the kernel needs no
// ordering of global memory between its threads.  The empty clusters are
// those of `counts` (a repair never empties a cluster or fills a later one).
__global__ __launch_bounds__(KM_FIN_THREADS) void k_km_finish(const int64_t* __restrict__ counts, int64_t k, int d,
                                                              float* __restrict__ cent, int64_t* __restrict__ h,
                                                              int64_t* __restrict__ n_split) {
    constexpr int NW = KM_FIN_THREADS / 64;
    constexpr float EPS = 1.0f / 1024.0f;
    __shared__ unsigned long long emask[NW];
    __shared__ long long wbest_h[NW];
    __shared__ long long wbest_c[NW];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int64_t nsplit = 0;
    for (int64_t base = 0; base < k; base += KM_FIN_THREADS) {
        const int64_t cme = base + t;
        const unsigned long long m = __ballot(cme < k && counts[cme] <= 0);
        if (lane == 0) emask[wave] = m;
        __syncthreads();
        for (int w = 0; w < NW; ++w) {
            unsigned long long mm = emask[w];
            while (mm) {
                const int64_t ci = base + w * 64 + __builtin_ctzll(mm);
                mm &= mm - 1;
                // the donor: the largest working count, ties to the smaller index
                long long bh = 0, bc = -1;
                for (int64_t c = t; c < k; c += KM_FIN_THREADS) {
                    const long long v = h[c];
                    if (v > bh) bh = v, bc = c;
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const long long oh = __shfl_xor(bh, o, 64), oc = __shfl_xor(bc, o, 64);
                    if (oh > bh || (oh == bh && oh > 0 && oc < bc)) bh = oh, bc = oc;
                }
                if (lane == 0) wbest_h[wave] = bh, wbest_c[wave] = bc;
                __syncthreads();
                bh = wbest_h[0], bc = wbest_c[0];
                for (int q = 1; q < NW; ++q) {
                    const long long oh = wbest_h[q], oc = wbest_c[q];
                    if (oh > bh || (oh == bh && oh > 0 && oc < bc)) bh = oh, bc = oc;
                }
                if (bh > 0) {  // (no cluster has a member: nothing to split)
                    const int64_t cj = bc;
                    for (int j = t; j < d; j += KM_FIN_THREADS) {
                        const float v = cent[cj * d + j];
                        const float up = v * (1.0f + EPS), dn = v * (1.0f - EPS);
                        cent[ci * d + j] = (j & 1) ? dn : up;
                        cent[cj * d + j] = (j & 1) ? up : dn;
                    }
                    if ((int)(ci % KM_FIN_THREADS) == t) h[ci] = bh / 2;
                    if ((int)(cj % KM_FIN_THREADS) == t) h[cj] = bh - bh / 2;
                    ++nsplit;
                }
                __syncthreads();  // (wbest_* are free again)
            }
        }
        __syncthreads();  // (emask is free again)
    }
    if (t == 0) *n_split = nsplit;
}

__global__ __launch_bounds__(KM_THREADS) void k_km_normalize(int64_t k, int d, float* __restrict__ cent) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * (KM_THREADS / 64) + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * (KM_THREADS / 64);
    for (int64_t c = wave; c < k; c += nwaves) {
        float* row = cent + c * d;
        double s = 0.0;
        for (int j = lane; j < d; j += 64) s += (double)row[j] * (double)row[j];
        s = wave_sum_f64(s);
        if (s > 0.0) {
            const double nrm = sqrt(s);
            for (int j = lane; j < d; j += 64) row[j] = (float)((double)row[j] / nrm);
        }
    }
}

hipError_t km_workspace(int64_t n, int64_t k, int d, size_t* bytes) {
    KmCarve c;
    const hipError_t e = km_carve(n, k, d, &c);
    if (e == hipSuccess) *bytes = c.total;
    return e;
}

hipError_t launch_km_update(const KmUpdate& u, void* ws, size_t ws_bytes, hipStream_t s, hipEvent_t mid) {
    if (u.n <= 0) return hipSuccess;
    if (!u.x || !u.assign || !u.sums || !u.counts || !u.obj || !u.bad || u.d <= 0 || u.k <= 0 ||
        u.n > (int64_t)INT32_MAX || u.k > (int64_t)INT32_MAX)
        return hipErrorInvalidValue;
    KmCarve c;
    hipError_t e = km_carve(u.n, u.k, u.d, &c);
    if (e != hipSuccess) return e;
    if (!ws || ws_bytes < c.total) return hipErrorInvalidValue;
    char* base = (char*)ws;
    uint64_t* keys = (uint64_t*)(base + c.keys);
    uint64_t* sorted = (uint64_t*)(base + c.sorted);
    int* seg = (int*)(base + c.seg);
    int* nblk = (int*)(base + c.nblk);
    int* blk0 = (int*)(base + c.blk0);
    double* objp = (double*)(base + c.objp);
    double* partial = (double*)(base + c.partial);
    hipLaunchKernelGGL(k_km_keys, dim3(km_grid(u.n, KM_THREADS)), dim3(KM_THREADS), 0, s, u.assign, u.n, u.k, keys,
                       u.bad);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t tb = c.temp_bytes;
    e = hipcub::DeviceRadixSort::SortKeys(base + c.temp, tb, (const uint64_t*)keys, sorted, (int)u.n, KM_SORT_BEGIN,
                                          32 + km_bits(u.k), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_km_seg, dim3(km_grid(u.k + 1, KM_THREADS)), dim3(KM_THREADS), 0, s, sorted, (int)u.n, u.k, seg,
                       nblk);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    tb = c.temp_bytes;
    e = hipcub::DeviceScan::ExclusiveSum(base + c.temp, tb, (const int*)nblk, blk0, (int)(u.k + 1), s);
    if (e != hipSuccess) return e;
    if (mid && (e = hipEventRecord(mid, s)) != hipSuccess) return e;
    // whole 16-B slices: the rows keep the base's alignment and no slice straddles d
    const int es = dtype_size(u.x_dt);
    const bool vec = ((int64_t)u.d * es) % 16 == 0 && ((uintptr_t)u.x & 15) == 0;
    const unsigned sgrid = (unsigned)std::min<int64_t>(c.max_blocks, KM_SUM_GRID_CAP);
    e = dispatch_dt_metric<DT_STORED>(u.x_dt, L2, [&](auto dtc, auto) {
        constexpr int DT = decltype(dtc)::value;
        if (vec)
            hipLaunchKernelGGL((k_km_sum<DT, true>), dim3(sgrid), dim3(KM_THREADS), 0, s, (const char*)u.x, u.n, u.d,
                               sorted, seg, blk0, u.k, partial);
        else
            hipLaunchKernelGGL((k_km_sum<DT, false>), dim3(sgrid), dim3(KM_THREADS), 0, s, (const char*)u.x, u.n, u.d,
                               sorted, seg, blk0, u.k, partial);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    int obj_blocks = 0;
    if (u.dist) {
        obj_blocks = c.obj_blocks;
        hipLaunchKernelGGL(k_km_obj, dim3(obj_blocks), dim3(KM_THREADS), 0, s, u.dist, u.assign, u.n, u.k, objp);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const int64_t items = u.k * ((u.d + KM_THREADS - 1) / KM_THREADS);
    hipLaunchKernelGGL(k_km_fold, dim3(km_grid(items, 1) + 1), dim3(KM_THREADS), 0, s, partial, seg, blk0, u.k, u.d,
                       u.sums, u.counts, objp, obj_blocks, u.obj, u.accumulate);
    return hipGetLastError();
}

hipError_t launch_km_finish(const KmFinish& f, hipStream_t s) {
    if (f.k <= 0 || f.d <= 0 || !f.sums || !f.counts || !f.codes || !f.cent || !f.h || !f.n_split)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_km_mean, dim3(km_grid(f.k * f.d, KM_THREADS)), dim3(KM_THREADS), 0, s, f.sums, f.counts, f.k,
                       f.d, f.codes, f.st_dt, f.row_bytes, f.cent, f.h);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_km_finish, dim3(1), dim3(KM_FIN_THREADS), 0, s, f.counts, f.k, f.d, f.cent, f.h, f.n_split);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (f.spherical) {
        hipLaunchKernelGGL(k_km_normalize, dim3(km_grid(f.k, KM_THREADS / 64)), dim3(KM_THREADS), 0, s, f.k, f.d,
                           f.cent);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace fx

// fx_range.hip -- range_search(): every row within a radius of each query.
//
// faiss IndexFlat::range_search(x, radius) returns, per query, every row y
// with D(q, y) < radius (L2; inner product: q.y > radius), as lims[nq + 1] and
// flat D / I arrays.  Membership is decided on the library's exact distance
// (fp64 sum in column order over the stored row, one rounding to fp32 -- the
// refine's, k_hk_keys' and the oracle's definition) against the fp32 radius;
// the MFMA pass only filters:
//
//   k_range_thr     per query, the scan key no row inside the radius can
//                   exceed (from k_prep_queries' bound: with a(y) the scan key
//                   of row y,  a(y) + s_q = D(y) + 2 r.(y - x) + err,
//                   |2 r.(y - x)| <= 2 rho sqrt(D(y)),  |err| <= E):
//                     L2:  T_q = R - s_q + 2 rho_q sqrt(R) + E_q
//                     IP:  T_q = -R + E_q
//                   in fp64, rounded up to fp32.  D < R implies a(y) < T_q, so
//                   the scan lets through false positives only.  An infinite
//                   E_q (overflowed fp16 operand) makes every row a candidate.
//   k_range_scan    the tile loop it shares with k_scan_topk (scan_tiles_128:
//                   128 rows x 128 queries, LDS-DMA double buffer, builtin
//                   MFMA) over the stored rows with
//                   |y|^2 (no centred / split image); epilogue: every live
//                   (query, existing row) pair with key <= T_q is appended to
//                   ONE global buffer as a packed (query << 32 | row) word.
//                   Space is reserved with one global atomic per wave per
//                   tile (and none when the wave has no candidate); the
//                   counter keeps counting past the buffer's capacity, entries
//                   past it are not stored (the host grows the buffer to the
//                   count and scans once more).
//   k_range_verify  one candidate per thread: the exact distance, the strict
//                   test; a failing word becomes the all-ones sentinel.
//   (radix sort)    hipCUB SortPairs of (word, D) over the used bits (the row's
//                   32 and the query's): the survivors in (query, row) order
//                   in front of the sentinels.
//   k_range_lims    lims[q] = first sorted word of query q (binary search).
//   k_range_ids     I = row + id_offset (a labelled index: the row's label).
#include "fx_device.h"

#include <hipcub/hipcub.hpp>

namespace fx {

constexpr int RG_THREADS = 256;
constexpr int LDS_RANGE_BYTES = LDS_LD_OFF;  // the stage double buffer + 2 x 512 B row norms
constexpr unsigned long long RG_NONE = ~0ull;  // a candidate the exact test removed

__global__ __launch_bounds__(RG_THREADS) void k_range_thr(int64_t nq, int metric, float radius,
                                                          const float* __restrict__ qeps,
                                                          const float* __restrict__ qrho,
                                                          const double* __restrict__ qshift,
                                                          float* __restrict__ thr) {
    const int64_t q = (int64_t)blockIdx.x * RG_THREADS + threadIdx.x;
    if (q >= nq) return;
    const double R = (double)radius, E = (double)qeps[q];
    double T = metric == L2 ? R - qshift[q] + 2.0 * (double)qrho[q] * sqrt(R) + E : -R + E;
    T += 1e-15 * fabs(T);                   // the fp64 roundings of the sum above
    if (!(T == T)) T = (double)FX_INF;      // no usable bound: every row is verified exactly
    float f = (float)T;
    if ((double)f < T) f = nextafterf(f, FX_INF);
    thr[q] = f;
}

template <int DT, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS, 1) void k_range_scan(ScanParams p, const float* __restrict__ thr,
                                                                unsigned long long* __restrict__ out,
                                                                unsigned long long cap,
                                                                unsigned long long* __restrict__ counter) {
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    int qtile, split;
    map_block(blockIdx.x, p, qtile, split);
    if (qtile >= p.n_qtiles || split >= p.splits || (int64_t)qtile * TILE_Q >= p.nq) return;
    const int64_t q0 = (int64_t)qtile * TILE_Q;

    // this lane's 4 query columns: live flag and threshold (fixed for the block)
    const int qcol = tile_qloc(0);  // + 16 n
    float tn[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int64_t q = q0 + qcol + n * 16;
        tn[n] = q < p.nq ? thr[q] : -FX_INF;  // a padding query takes no row
    }

    // per finished tile: filter against T_q, append.  (always_inline: the epilogue must become part of
    // the loop's body, or the accumulators it reads go through scratch)
    scan_tiles_128<DT, METRIC>(p, smem, qtile, split, [&](const auto& acc, const auto& yn, int trow0, int rlim, int rl0)
                                                          __attribute__((always_inline)) {
        // bit n * 16 + m * 4 + i: the pair (query column n, row m * 16 + i) passes
        unsigned long long mask = 0ull;
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = METRIC == L2 ? acc[m][n][i] + yn[m][i] : acc[m][n][i];
                    const int rl = tile_rloc(rl0, m, i);
                    if (rl < rlim && v <= tn[n]) mask |= 1ull << (n * 16 + m * 4 + i);
                }
        const int c = __popcll(mask);
        if (__any(c != 0)) {  // (wave-uniform) one reservation for the wave's candidates of this tile
            int incl = c;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int up = __shfl_up(incl, o, 64);
                if (lane >= o) incl += up;
            }
            const int total = __shfl(incl, 63, 64);
            unsigned long long base = 0ull;
            if (lane == 0) base = atomicAdd(counter, (unsigned long long)total);
            const unsigned blo = __builtin_amdgcn_readfirstlane((unsigned)(base & 0xffffffffull));
            const unsigned bhi = __builtin_amdgcn_readfirstlane((unsigned)(base >> 32));
            unsigned long long pos = (((unsigned long long)bhi << 32) | blo) + (unsigned long long)(incl - c);
            while (mask) {
                const int e = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const unsigned long long q = (unsigned long long)(q0 + qcol + (e >> 4) * 16);
                const unsigned row = (unsigned)(trow0 + tile_rloc(rl0, (e >> 2) & 3, e & 3));
                if (pos < cap) out[pos] = (q << 32) | row;
                ++pos;
            }
        }
    });
}

// the exact test of what the scan let through: one candidate per thread, the
// arithmetic of the refine and k_hk_keys (exact_partial: fp64 fma chain in
// column order, one rounding)
template <int DT, int METRIC>
__global__ __launch_bounds__(RG_THREADS) void k_range_verify(unsigned long long* __restrict__ words, int64_t n,
                                                             const char* __restrict__ codes, int row_bytes, int kdim,
                                                             int64_t ntotal, const float* __restrict__ qf32,
                                                             int64_t nq, float radius, float* __restrict__ dist,
                                                             int* __restrict__ n_drop) {
    const int64_t i = (int64_t)blockIdx.x * RG_THREADS + threadIdx.x;
    if (i >= n) return;
    const unsigned long long w = words[i];
    const int64_t q = (int64_t)(w >> 32), row = (int64_t)(w & 0xffffffffull);
    if (q >= nq || row >= ntotal) {  // a corrupted word: never gathered, counted
        atomicAdd(n_drop, 1);
        words[i] = RG_NONE;
        dist[i] = 0.f;
        return;
    }
    const float f = (float)exact_partial<DT, METRIC>(qf32 + q * kdim, codes + row * row_bytes, row_bytes, 0, 1);
    dist[i] = f;
    if (!(METRIC == L2 ? f < radius : f > radius)) words[i] = RG_NONE;
}

// lims[q] = index of the first sorted word of a query >= q, q = 0 .. nq
// (lims[nq] = the number of survivors: the sentinels sort last)
__global__ __launch_bounds__(RG_THREADS) void k_range_lims(const unsigned long long* __restrict__ sorted, int64_t n,
                                                           int64_t nq, int64_t* __restrict__ lims) {
    const int64_t q = (int64_t)blockIdx.x * RG_THREADS + threadIdx.x;
    if (q > nq) return;
    const unsigned long long key = (unsigned long long)q << 32;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (sorted[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    lims[q] = lo;
}

__global__ __launch_bounds__(RG_THREADS) void k_range_ids(const unsigned long long* __restrict__ sorted,
                                                          const int64_t* __restrict__ lims, int64_t nq,
                                                          int64_t id_offset, const int64_t* __restrict__ labels,
                                                          int64_t* __restrict__ I) {
    const int64_t total = lims[nq];
    for (int64_t i = (int64_t)blockIdx.x * RG_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * RG_THREADS)
        I[i] = result_id(labels, (int64_t)(sorted[i] & 0xffffffffull), id_offset);
}

namespace {

// bits of a candidate word the sort has to look at: the row's 32 and as many
// query bits as make the all-ones sentinel's query field exceed every query
int rg_sort_bits(int64_t nq) {
    int b = 1;
    while (b < 32 && ((int64_t)1 << b) <= nq) ++b;
    return 32 + b;
}

unsigned rg_blocks(int64_t items) { return (unsigned)std::max<int64_t>(1, (items + RG_THREADS - 1) / RG_THREADS); }

}  // namespace

hipError_t launch_range_thr(int64_t nq, int metric, float radius, const float* qeps, const float* qrho,
                            const double* qshift, float* thr, hipStream_t s) {
    hipLaunchKernelGGL(k_range_thr, dim3(rg_blocks(nq)), dim3(RG_THREADS), 0, s, nq, metric, radius, qeps, qrho,
                       qshift, thr);
    return hipGetLastError();
}

hipError_t launch_range_scan(int st_dt, int metric, const ScanParams& p, const float* thr, uint64_t* cand,
                             uint64_t cap, uint64_t* counter, hipStream_t s) {
    if (p.row_bytes <= 0 || p.row_bytes % STAGE_B != 0 || p.grid <= 0 || p.qt != TILE_Q || p.tr != TILE_R)
        return hipErrorInvalidValue;
    return dispatch_dt_metric<DT_STORED>(st_dt, metric, [&](auto dt, auto mt) {
        return launch_with_lds(k_range_scan<dt(), mt()>, p.grid, SCAN_THREADS, LDS_RANGE_BYTES, s, p, thr,
                               (unsigned long long*)cand, (unsigned long long)cap, (unsigned long long*)counter);
    });
}

hipError_t range_sort_temp_bytes(int64_t n, int64_t nq, size_t* bytes) {
    *bytes = 0;
    if (n <= 0 || n > INT_MAX) return hipErrorInvalidValue;
    return hipcub::DeviceRadixSort::SortPairs(nullptr, *bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                              (const float*)nullptr, (float*)nullptr, (int)n, 0,
                                              rg_sort_bits(nq), (hipStream_t)0);
}

hipError_t launch_range_finish(const RangeFinish& f, hipStream_t s) {
    if (f.n <= 0 || f.n > INT_MAX || f.nq <= 0) return hipErrorInvalidValue;
    hipError_t e = dispatch_dt_metric<DT_STORED>(f.st_dt, f.metric, [&](auto dt, auto mt) {
        hipLaunchKernelGGL((k_range_verify<dt(), mt()>), dim3(rg_blocks(f.n)), dim3(RG_THREADS), 0, s,
                           (unsigned long long*)f.words, f.n, f.codes, f.row_bytes, f.kdim, f.ntotal, f.qf32, f.nq,
                           f.radius, f.dist, f.n_drop);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    size_t tb = f.temp_bytes;
    e = hipcub::DeviceRadixSort::SortPairs(f.temp, tb, (const uint64_t*)f.words, f.sorted, (const float*)f.dist, f.D,
                                           (int)f.n, 0, rg_sort_bits(f.nq), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_range_lims, dim3(rg_blocks(f.nq + 1)), dim3(RG_THREADS), 0, s,
                       (const unsigned long long*)f.sorted, f.n, f.nq, f.lims);
    hipLaunchKernelGGL(k_range_ids, dim3(std::min(rg_blocks(f.n), 4096u)), dim3(RG_THREADS), 0, s,
                       (const unsigned long long*)f.sorted, (const int64_t*)f.lims, f.nq, f.id_offset, f.labels, f.I);
    return hipGetLastError();
}

}  // namespace fx

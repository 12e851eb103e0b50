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
//   k_range_scan    k_scan_topk's tile loop (128 rows x 128 queries, LDS-DMA
//                   double buffer, builtin MFMA) over the stored rows with
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
//   k_range_ids     I = row + id_offset.
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
    typedef typename Frag<DT>::T frag_t;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    int qtile, split;
    map_block(blockIdx.x, p, qtile, split);
    if (qtile >= p.n_qtiles || split >= p.splits || (int64_t)qtile * TILE_Q >= p.nq) return;
    const int ct0 = (int)((int64_t)split * p.n_ctiles / p.splits);
    const int ct1 = (int)((int64_t)(split + 1) * p.n_ctiles / p.splits);
    const int nks = p.row_bytes / STAGE_B;
    const int G = (ct1 - ct0) * nks;
    const int64_t q0 = (int64_t)qtile * TILE_Q;
    const int rb = p.row_bytes;

    // per-lane byte offsets of this wave's 4 A blocks and 4 B blocks inside a
    // tile (block bi = 16-row block * 2 + 64-B half), as k_scan_topk
    int offs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int bi = wave * 4 + j, rblk = bi >> 1, kb = bi & 1;
        offs[j] = (rblk * 16 + (lane & 15)) * rb + kb * 64 + (lane >> 4) * 16;
    }
    const char* qbase = p.qop + q0 * rb;

    auto issue = [&](int g) {
        const int t = g / nks, ks = g - t * nks;
        char* buf = smem + (g & 1) * ((TILE_R + TILE_Q) * STAGE_B);
        const int64_t row0 = (int64_t)(ct0 + t) * TILE_R;
        const char* abase = p.codes + row0 * rb + ks * STAGE_B;
        const char* bbase = qbase + ks * STAGE_B;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            glds16(abase + offs[j], buf + (wave * 4 + j) * 1024);
            glds16(bbase + offs[j], buf + TILE_R * STAGE_B + (wave * 4 + j) * 1024);
        }
        if (METRIC == L2 && ks == 0 && wave == 0 && lane < 32)
            glds16(p.norms + row0 + lane * 4, smem + LDS_NORM_OFF + (t & 1) * (TILE_R * 4));
    };

    // this lane's 4 query columns: live flag and threshold (fixed for the block)
    const int qcol = wn * 64 + (lane & 15);  // + 16 n
    float tn[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const int64_t q = q0 + qcol + n * 16;
        tn[n] = q < p.nq ? thr[q] : -FX_INF;  // a padding query takes no row
    }

    f32x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (G > 0) issue(0);
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");

    int t = 0, ks = 0;
    for (int g = 0; g < G; ++g) {
        if (g + 1 < G) issue(g + 1);
        const char* buf = smem + (g & 1) * ((TILE_R + TILE_Q) * STAGE_B);
#pragma unroll
        for (int kb = 0; kb < 2; ++kb) {
            frag_t a[4], b[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) a[m] = *(const frag_t*)(buf + ((wm * 4 + m) * 2 + kb) * 1024 + lane * 16);
#pragma unroll
            for (int n = 0; n < 4; ++n)
                b[n] = *(const frag_t*)(buf + TILE_R * STAGE_B + ((wn * 4 + n) * 2 + kb) * 1024 + lane * 16);
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[m][n] = Frag<DT>::mma(a[m], b[n], acc[m][n]);
        }

        if (ks == nks - 1) {
            // ---------------- epilogue: filter against T_q, append --------------
            const float* nb = (const float*)(smem + LDS_NORM_OFF + (t & 1) * (TILE_R * 4));
            const int trow0 = (ct0 + t) * TILE_R;
            const int rlim = (int)(p.ntotal - (int64_t)trow0);  // rows of this tile that exist
            const int rl0 = wm * 64 + 4 * (lane >> 4);           // local row of (m = 0, i = 0)
            float yn[4][4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (METRIC == L2) {
                    float4 v = *(const float4*)(nb + rl0 + m * 16);
                    yn[m][0] = v.x; yn[m][1] = v.y; yn[m][2] = v.z; yn[m][3] = v.w;
                } else {
                    yn[m][0] = yn[m][1] = yn[m][2] = yn[m][3] = 0.f;
                }
            }
            // bit n * 16 + m * 4 + i: the pair (query column n, row m * 16 + i) passes
            unsigned long long mask = 0ull;
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float v = METRIC == L2 ? acc[m][n][i] + yn[m][i] : acc[m][n][i];
                        const int rl = rl0 + m * 16 + i;
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
                    const unsigned row = (unsigned)(trow0 + rl0 + ((e >> 2) & 3) * 16 + (e & 3));
                    if (pos < cap) out[pos] = (q << 32) | row;
                    ++pos;
                }
            }
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
            ks = 0;
            ++t;
        } else {
            ++ks;
        }
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    }
}

// the exact test of what the scan let through: one candidate per thread, the
// arithmetic of k_hk_keys (fp64 fma chain in column order, one rounding)
template <int DT, int METRIC>
__global__ __launch_bounds__(RG_THREADS) void k_range_verify(unsigned long long* __restrict__ words, int64_t n,
                                                             const char* __restrict__ codes, int row_bytes, int kdim,
                                                             int64_t ntotal, const float* __restrict__ qf32,
                                                             int64_t nq, float radius, float* __restrict__ dist,
                                                             int* __restrict__ n_drop) {
    constexpr int E = DT == F32 ? 4 : 8;
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
    const char* yrow = codes + row * row_bytes;
    const float* xq = qf32 + q * kdim;
    double acc = 0.0;
    for (int c = 0; c * 16 < row_bytes; ++c) {
        float y[E];
        load_chunk<DT>(yrow + c * 16, y);
        const float* xc = xq + c * E;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if (METRIC == L2) {
                const double df = (double)xc[e] - (double)y[e];
                acc = fma(df, df, acc);
            } else {
                acc = fma((double)xc[e], (double)y[e], acc);
            }
        }
    }
    const float f = (float)acc;
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
                                                          int64_t id_offset, int64_t* __restrict__ I) {
    const int64_t total = lims[nq];
    for (int64_t i = (int64_t)blockIdx.x * RG_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * RG_THREADS)
        I[i] = (int64_t)(sorted[i] & 0xffffffffull) + id_offset;
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

template <int DT, int METRIC>
hipError_t range_scan_t(const ScanParams& p, const float* thr, unsigned long long* out, unsigned long long cap,
                        unsigned long long* counter, hipStream_t s) {
    // > 64 KiB of dynamic LDS must be opted into (per device; cheap to repeat)
    hipError_t e = hipFuncSetAttribute((const void*)k_range_scan<DT, METRIC>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, LDS_RANGE_BYTES);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_range_scan<DT, METRIC>), dim3(p.grid), dim3(SCAN_THREADS), LDS_RANGE_BYTES, s, p, thr, out,
                       cap, counter);
    return hipGetLastError();
}

template <int DT, int METRIC>
void range_verify_t(const RangeFinish& f, hipStream_t s) {
    hipLaunchKernelGGL((k_range_verify<DT, METRIC>), dim3(rg_blocks(f.n)), dim3(RG_THREADS), 0, s,
                       (unsigned long long*)f.words, f.n, f.codes, f.row_bytes, f.kdim, f.ntotal, f.qf32, f.nq,
                       f.radius, f.dist, f.n_drop);
}

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
    unsigned long long* out = (unsigned long long*)cand;
    unsigned long long* cnt = (unsigned long long*)counter;
    if (metric == L2) {
        if (st_dt == F32) return range_scan_t<F32, L2>(p, thr, out, cap, cnt, s);
        if (st_dt == BF16) return range_scan_t<BF16, L2>(p, thr, out, cap, cnt, s);
        if (st_dt == F16) return range_scan_t<F16, L2>(p, thr, out, cap, cnt, s);
        return hipErrorInvalidValue;
    }
    if (st_dt == F32) return range_scan_t<F32, IP>(p, thr, out, cap, cnt, s);
    if (st_dt == BF16) return range_scan_t<BF16, IP>(p, thr, out, cap, cnt, s);
    if (st_dt == F16) return range_scan_t<F16, IP>(p, thr, out, cap, cnt, s);
    return hipErrorInvalidValue;
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
    if (f.metric == L2) {
        if (f.st_dt == F32) range_verify_t<F32, L2>(f, s);
        else if (f.st_dt == BF16) range_verify_t<BF16, L2>(f, s);
        else range_verify_t<F16, L2>(f, s);
    } else {
        if (f.st_dt == F32) range_verify_t<F32, IP>(f, s);
        else if (f.st_dt == BF16) range_verify_t<BF16, IP>(f, s);
        else range_verify_t<F16, IP>(f, s);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t tb = f.temp_bytes;
    e = hipcub::DeviceRadixSort::SortPairs(f.temp, tb, (const uint64_t*)f.words, f.sorted, (const float*)f.dist, f.D,
                                           (int)f.n, 0, rg_sort_bits(f.nq), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_range_lims, dim3(rg_blocks(f.nq + 1)), dim3(RG_THREADS), 0, s,
                       (const unsigned long long*)f.sorted, f.n, f.nq, f.lims);
    hipLaunchKernelGGL(k_range_ids, dim3(std::min(rg_blocks(f.n), 4096u)), dim3(RG_THREADS), 0, s,
                       (const unsigned long long*)f.sorted, (const int64_t*)f.lims, f.nq, f.id_offset, f.I);
    return hipGetLastError();
}

}  // namespace fx

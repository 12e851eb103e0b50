// fx_ivf.hip -- inverted file: faiss's IndexIVFFlat over a list-ordered payload.
//
// The payload is a labelled flat index whose rows lie in LIST ORDER: list l owns
// rows [list_off[l], list_off[l + 1]), in insertion order.  A search probes, per
// query, the nprobe lists its coarse search names, and ranks their rows exactly.
//
//   k_ivf_rkeys / k_ivf_offsets / k_ivf_gather_*   the regroup after an add: a
//                stable radix sort of list << 32 | row keys by the list bits,
//                the lists' first rows, and the gather of codes (bitwise),
//                norms, labels and list numbers into second buffers.
//   k_ivf_pkeys / k_ivf_groups   the (query, probed list) pairs of a pass as
//                list << 32 | pair keys, sorted by list; per list the first
//                sorted position and its query groups ceil(count / 128), whose
//                exclusive scan numbers the groups.  All on the device.
//   k_ivf_scan   one workgroup per (query group, tile chunk): the 128 x 128 MFMA
//                tile loop (a sibling of scan_tiles_128, fx_device.h) over the
//                list's rows where they lie -- tile starts aligned down to 4
//                rows, rows outside the list masked by row number -- against the
//                group's queries, whose operands are fetched through the sorted
//                pairs by per-lane global addresses (no gathered copy).  The
//                epilogue is k_scan_topk's LDS lists; the flush writes the
//                sorted top-KP of (item, query) to cand[q][j C + chunk][KP].
//   k_ivf_exact / k_ivf_merge   the exact path: fp64 distances of every row of a
//                probed list chunk, block top-k, then the per-query merge under
//                (key, row).  Serves the queries the refine flags (k <= KP) and
//                the whole search for KP < k <= FX_BIG_K.
#include "fx_device.h"

#include <hipcub/hipcub.hpp>

#include <algorithm>

namespace fx {

namespace {

constexpr int IVF_THREADS = 256;
constexpr int IVF_GRID_CAP = 4096;
constexpr int IVF_SORT_BEGIN = 32;  // keys are sorted by their list bits only (a stable sort)
constexpr int IVF_EXACT_GRID = 1024, IVF_MERGE_GRID = 256;
// LDS of k_ivf_scan: k_scan_topk's carve, then the group's pair numbers
constexpr int LDS_IVF_PAIR_OFF = LDS_SCAN_BYTES;
constexpr int LDS_IVF_BYTES = LDS_IVF_PAIR_OFF + TILE_Q * 4;

inline size_t ivf_align(size_t v) { return (v + 255) / 256 * 256; }

// bits that hold a list number 0 .. nlist (nlist: the segment of the invalid entries)
inline int ivf_bits(int64_t nlist) {
    int b = 1;
    while (((int64_t)1 << b) <= nlist) ++b;
    return b;
}

unsigned ivf_grid(int64_t items, int per_block) {
    const int64_t g = (items + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : g > IVF_GRID_CAP ? IVF_GRID_CAP : g);
}

hipError_t ivf_sort_temp(int64_t n, int64_t nlist, size_t* bytes) {
    size_t sort_tb = 0, scan_tb = 0;
    hipError_t e = hipcub::DeviceRadixSort::SortKeys(nullptr, sort_tb, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                                     (int)n, IVF_SORT_BEGIN, 32 + ivf_bits(nlist));
    if (e != hipSuccess) return e;
    e = hipcub::DeviceScan::ExclusiveSum(nullptr, scan_tb, (const int*)nullptr, (int*)nullptr, (int)(nlist + 1));
    if (e != hipSuccess) return e;
    *bytes = std::max(sort_tb, scan_tb);
    return hipSuccess;
}

}  // namespace

// first position of `sorted` whose list is >= l
__device__ __forceinline__ int ivf_lower(const uint64_t* __restrict__ sorted, int n, int64_t l) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((int64_t)(sorted[mid] >> 32) < l) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------
// add: the rows' lists, sequential ids
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(IVF_THREADS) void k_ivf_record(const int64_t* __restrict__ assign, int64_t n,
                                                            int64_t nlist, int* __restrict__ row_list,
                                                            unsigned long long* __restrict__ bad) {
    for (int64_t i = (int64_t)blockIdx.x * IVF_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IVF_THREADS) {
        const int64_t a = assign[i];
        const bool ok = a >= 0 && a < nlist;
        row_list[i] = (int)(ok ? a : nlist);
        if (!ok) atomicAdd(bad, 1ull);
    }
}

__global__ __launch_bounds__(IVF_THREADS) void k_ivf_iota(int64_t* __restrict__ ids, int64_t n, int64_t first) {
    for (int64_t i = (int64_t)blockIdx.x * IVF_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IVF_THREADS)
        ids[i] = first + i;
}

// ---------------------------------------------------------------------------
// regroup
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(IVF_THREADS) void k_ivf_rkeys(const int* __restrict__ row_list, int64_t n, int64_t nlist,
                                                           uint64_t* __restrict__ keys) {
    for (int64_t i = (int64_t)blockIdx.x * IVF_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IVF_THREADS) {
        const int l = row_list[i];
        const bool ok = l >= 0 && l < nlist;
        keys[i] = (uint64_t)(ok ? l : nlist) << 32 | (uint32_t)i;
    }
}

__global__ __launch_bounds__(IVF_THREADS) void k_ivf_offsets(const uint64_t* __restrict__ sorted, int n,
                                                             int64_t nlist, int* __restrict__ list_off,
                                                             int* __restrict__ max_rows) {
    for (int64_t l = (int64_t)blockIdx.x * IVF_THREADS + threadIdx.x; l <= nlist;
         l += (int64_t)gridDim.x * IVF_THREADS) {
        const int s0 = ivf_lower(sorted, n, l);
        list_off[l] = s0;
        if (l < nlist) atomicMax(max_rows, ivf_lower(sorted, n, l + 1) - s0);
    }
}

// dst row i <- src row (sorted[i] & 0xffffffff), 16 B per thread
__global__ __launch_bounds__(IVF_THREADS) void k_ivf_gather_codes(const uint64_t* __restrict__ sorted, int64_t n,
                                                                  int cpr /* 16-B chunks per row */,
                                                                  const uint4* __restrict__ src,
                                                                  uint4* __restrict__ dst) {
    const int64_t items = n * cpr;
    for (int64_t x = (int64_t)blockIdx.x * IVF_THREADS + threadIdx.x; x < items;
         x += (int64_t)gridDim.x * IVF_THREADS) {
        const int64_t i = x / cpr;
        const int c = (int)(x - i * cpr);
        const int64_t r = (int64_t)(uint32_t)sorted[i];
        dst[i * cpr + c] = r < n ? src[r * cpr + c] : make_uint4(0u, 0u, 0u, 0u);
    }
}

__global__ __launch_bounds__(IVF_THREADS) void k_ivf_gather_meta(const uint64_t* __restrict__ sorted, int64_t n,
                                                                 const float* __restrict__ norms,
                                                                 const int64_t* __restrict__ labels,
                                                                 float* __restrict__ dst_norms,
                                                                 int64_t* __restrict__ dst_labels,
                                                                 int* __restrict__ dst_row_list) {
    for (int64_t i = (int64_t)blockIdx.x * IVF_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IVF_THREADS) {
        const uint64_t key = sorted[i];
        const int64_t r = (int64_t)(uint32_t)key;
        if (r >= n) continue;  // (never: the keys' row halves are a permutation of [0, n))
        dst_norms[i] = norms[r];
        dst_labels[i] = labels[r];
        dst_row_list[i] = (int)(key >> 32);
    }
}

// ---------------------------------------------------------------------------
// pairs
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(IVF_THREADS) void k_ivf_pkeys(const int64_t* __restrict__ coarse, int64_t npairs,
                                                           int64_t nlist, uint64_t* __restrict__ keys,
                                                           int* __restrict__ bad) {
    for (int64_t p = (int64_t)blockIdx.x * IVF_THREADS + threadIdx.x; p < npairs;
         p += (int64_t)gridDim.x * IVF_THREADS) {
        const int64_t l = coarse[p];
        const bool ok = l >= 0 && l < nlist;
        keys[p] = (uint64_t)(ok ? l : nlist) << 32 | (uint32_t)p;
        if (!ok) atomicAdd(bad, 1);
    }
}

__global__ __launch_bounds__(IVF_THREADS) void k_ivf_groups(const uint64_t* __restrict__ sorted, int npairs,
                                                            int64_t nlist, const int* __restrict__ list_off,
                                                            int* __restrict__ seg, int* __restrict__ ngrp) {
    for (int64_t l = (int64_t)blockIdx.x * IVF_THREADS + threadIdx.x; l <= nlist;
         l += (int64_t)gridDim.x * IVF_THREADS) {
        const int s0 = ivf_lower(sorted, npairs, l);
        seg[l] = s0;
        int g = 0;
        if (l < nlist && list_off[l + 1] > list_off[l]) g = (ivf_lower(sorted, npairs, l + 1) - s0 + TILE_Q - 1) / TILE_Q;
        ngrp[l] = g;
    }
}

// ---------------------------------------------------------------------------
// the list scan.  scan_tiles_ivf is scan_tiles_128 (fx_device.h) with the two
// operand sources of an inverted list: the A tiles are tiles [t0, t1) of 128
// rows from row a0 (a multiple of 4, so the norms' 16-B DMA stays aligned), and
// the B rows are taken per lane from boffs (byte offsets into qop of the
// query row that is column rblk * 16 + (lane & 15) of the tile).
// ep(acc, yn, trow0, rl0) as there; rows are masked by the caller.
// ---------------------------------------------------------------------------
template <int DT, int METRIC, class Epilogue>
__device__ __forceinline__ void scan_tiles_ivf(const IvfScan& p, char* smem, int64_t a0, int t0, int t1,
                                               const int64_t (&boffs)[4], Epilogue&& ep) {
    typedef typename Frag<DT>::T frag_t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int rb = p.row_bytes;
    const int nks = rb / STAGE_B;
    const int G = (t1 - t0) * nks;

    int offs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int bi = wave * 4 + j, rblk = bi >> 1, kb = bi & 1;
        offs[j] = (rblk * 16 + (lane & 15)) * rb + kb * 64 + (lane >> 4) * 16;
    }

    auto issue = [&](int g) {
        const int t = g / nks, ks = g - t * nks;
        char* buf = smem + (g & 1) * ((TILE_R + TILE_Q) * STAGE_B);
        const int64_t row0 = a0 + (int64_t)(t0 + t) * TILE_R;
        const char* abase = p.codes + row0 * rb + ks * STAGE_B;
        const char* bbase = p.qop + ks * STAGE_B;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            glds16(abase + offs[j], buf + (wave * 4 + j) * 1024);
            glds16(bbase + boffs[j], buf + TILE_R * STAGE_B + (wave * 4 + j) * 1024);
        }
        if (METRIC == L2 && ks == 0 && wave == 0 && lane < 32)
            glds16(p.norms + row0 + lane * 4, smem + LDS_NORM_OFF + (t & 1) * (TILE_R * 4));
    };

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

        if (__builtin_expect(ks == nks - 1, 0)) {
            const float* nb = (const float*)(smem + LDS_NORM_OFF + (t & 1) * (TILE_R * 4));
            const int64_t trow0 = a0 + (int64_t)(t0 + t) * TILE_R;
            const int rl0 = wm * 64 + 4 * (lane >> 4);
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
            ep(acc, yn, trow0, rl0);
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

template <int DT, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS, 1) void k_ivf_scan(IvfScan p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = (int)(blockIdx.x / (unsigned)p.C), chunk = (int)(blockIdx.x % (unsigned)p.C);
    const int nlist = (int)p.nlist;
    if (g >= p.gbase[nlist]) return;  // (blocks past the pass's group total)
    // the group's list: the first l with gbase[l + 1] > g (then gbase[l] <= g)
    int lo = 0, hi = nlist - 1;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (p.gbase[mid + 1] > g) hi = mid;
        else lo = mid + 1;
    }
    const int l = __builtin_amdgcn_readfirstlane(lo);
    const int r0 = __builtin_amdgcn_readfirstlane(p.list_off[l]);
    const int r1 = __builtin_amdgcn_readfirstlane(p.list_off[l + 1]);
    const int a0 = r0 & ~3;
    const int nt = (r1 - a0 + TILE_R - 1) / TILE_R;
    const int t0 = (int)((int64_t)nt * chunk / p.C), t1 = (int)((int64_t)nt * (chunk + 1) / p.C);
    if (r1 <= r0 || t0 >= t1) return;  // (its slots keep the -1 the host wrote)
    const int pos0 = __builtin_amdgcn_readfirstlane(p.seg[l]) + (g - __builtin_amdgcn_readfirstlane(p.gbase[l])) * TILE_Q;
    const int nqg = min(TILE_Q, __builtin_amdgcn_readfirstlane(p.seg[l + 1]) - pos0);  // the group's queries
    if (nqg <= 0) return;

    float* lst_d = (float*)(smem + LDS_LD_OFF);
    int* lst_i = (int*)(smem + LDS_LI_OFF);
    int* cnt = (int*)(smem + LDS_CNT_OFF);
    float* tau = (float*)(smem + LDS_TAU_OFF);
    volatile int* flag = (volatile int*)(smem + LDS_FLAG_OFF);
    unsigned* pair = (unsigned*)(smem + LDS_IVF_PAIR_OFF);

    for (int x = tid; x < TILE_Q; x += SCAN_THREADS) {
        cnt[x] = 0;
        tau[x] = FX_INF;
        pair[x] = x < nqg ? (unsigned)p.sorted[pos0 + x] : 0xffffffffu;
    }
    if (tid == 0) *flag = 0;
    __syncthreads();

    // the lane's four B rows: the query of column rblk * 16 + (lane & 15); a
    // column past the group reads query 0 of the pass (never pushed)
    int64_t boffs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int bi = wave * 4 + j, rblk = bi >> 1, kb = bi & 1;
        const unsigned pr = pair[rblk * 16 + (lane & 15)];
        const int64_t q = pr == 0xffffffffu ? 0 : (int64_t)(pr / (unsigned)p.np);
        boffs[j] = q * p.row_bytes + kb * 64 + (lane >> 4) * 16;
    }

    scan_tiles_ivf<DT, METRIC>(
        p, smem, (int64_t)a0, t0, t1, boffs,
        [&](const auto& acc, const auto& yn, int64_t trow0, int rl0) __attribute__((always_inline)) {
            int qloc[4];
            bool qv[4];
            float tn[4];
            unsigned pend[4];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                qloc[n] = tile_qloc(n);
                qv[n] = qloc[n] < nqg;
                tn[n] = tau[qloc[n]];
                pend[n] = 0u;
            }
            // rows of this lane that belong to the list: bit m * 4 + i
            unsigned sel = 0u;
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int64_t row = trow0 + tile_rloc(rl0, m, i);
                    if (row >= r0 && row < r1) sel |= 1u << (m * 4 + i);
                }
            int ovf = 0;
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float v = METRIC == L2 ? acc[m][n][i] + yn[m][i] : acc[m][n][i];
                        if (qv[n] && ((sel >> (m * 4 + i)) & 1u) && v <= tn[n]) {
                            const int s = atomicAdd(&cnt[qloc[n]], 1);
                            if (s < CAP) {
                                lst_d[qloc[n] * CAP + s] = v;
                                lst_i[qloc[n] * CAP + s] = (int)trow0 + tile_rloc(rl0, m, i);
                            } else {
                                pend[n] |= 1u << (m * 4 + i);
                                ovf = 1;
                            }
                        }
                    }
            if (ovf) *flag = 1;
            __syncthreads();
            while (*flag) {
                __syncthreads();
                if (tid == 0) *flag = 0;
                compact_full(lst_d, lst_i, cnt, tau, wave, lane);
                __syncthreads();
                ovf = 0;
#pragma unroll
                for (int n = 0; n < 4; ++n) {
                    tn[n] = tau[qloc[n]];
#pragma unroll
                    for (int m = 0; m < 4; ++m)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const unsigned bit = 1u << (m * 4 + i);
                            if (pend[n] & bit) {
                                const float v = METRIC == L2 ? acc[m][n][i] + yn[m][i] : acc[m][n][i];
                                pend[n] &= ~bit;
                                if (v <= tn[n]) {
                                    const int s = atomicAdd(&cnt[qloc[n]], 1);
                                    if (s < CAP) {
                                        lst_d[qloc[n] * CAP + s] = v;
                                        lst_i[qloc[n] * CAP + s] = (int)trow0 + tile_rloc(rl0, m, i);
                                    } else {
                                        pend[n] |= bit;
                                        ovf = 1;
                                    }
                                }
                            }
                        }
                }
                if (ovf) *flag = 1;
                __syncthreads();
            }
        });

    // final flush: the sorted top-KP of (this item, query) -> the query's slot j * C + chunk
    __syncthreads();
    const int slots = p.np * p.C;
    for (int q = wave; q < nqg; q += 4) {
        const unsigned pr = pair[q];
        const int64_t qq = (int64_t)(pr / (unsigned)p.np);
        const int j = (int)(pr % (unsigned)p.np);
        const int64_t obase = (qq * slots + (int64_t)j * p.C + chunk) * KP;
        const int c = min(cnt[q], CAP);
        float d = lane < c ? lst_d[q * CAP + lane] : FX_INF;
        int i = lane < c ? lst_i[q * CAP + lane] : INT_MAX;
        sort64(d, i, lane);
        if (lane < KP) {
            p.cand_d[obase + lane] = d;
            p.cand_i[obase + lane] = i == INT_MAX ? -1 : i;
        }
    }
}

// ---------------------------------------------------------------------------
// the exact path
// ---------------------------------------------------------------------------
template <int DT, int METRIC>
__global__ __launch_bounds__(BT_THREADS) void k_ivf_exact(IvfExact p) {
    __shared__ float sd[BT_MAXB];
    __shared__ int si[BT_MAXB];
    __shared__ BtState<int> st;
    const int nf = p.n_flag[0];
    if (nf <= 0) return;
    const int* qlist = p.n_flag + 1;
    const int slots = p.np * p.C, B = bt_cap(p.k);
    const int64_t items = (int64_t)nf * slots;
    for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const int f = (int)(w / slots), slot = (int)(w % slots);
        const int j = slot / p.C, c = slot % p.C;
        const int64_t q = qlist[f];
        const float* xq = p.qf32 + q * p.kdim;
        const int64_t l = p.coarse[q * p.np + j];
        int64_t a = 0, b = 0;  // the chunk's rows (none for a list number outside the index)
        if (l >= 0 && l < p.nlist) {
            const int64_t r0 = p.list_off[l], r1 = p.list_off[l + 1];
            a = r0 + (r1 - r0) * c / p.C;
            b = r0 + (r1 - r0) * (c + 1) / p.C;
        }
        bt_init(&st);
        for (int64_t base = a; base < b; base += BT_THREADS) {
            const int64_t row = base + threadIdx.x;
            const bool valid = row < b;
            float key = FX_INF;
            if (valid) {
                const double v = exact_partial<DT, METRIC>(xq, p.codes + row * p.row_bytes, p.row_bytes, 0, 1);
                key = METRIC == L2 ? (float)v : -(float)v;
            }
            bt_round(sd, si, &st, p.k, B, key, valid ? (int)row : INT_MAX, valid);
        }
        bt_flush(sd, si, &st, p.k, B);
        const int cn = st.cnt;
        for (int t = threadIdx.x; t < p.k; t += BT_THREADS) {
            p.cd[w * p.k + t] = t < cn ? sd[t] : FX_INF;
            p.ci[w * p.k + t] = t < cn ? si[t] : -1;
        }
        __syncthreads();
    }
}

template <int METRIC>
__global__ __launch_bounds__(BT_THREADS) void k_ivf_merge(IvfExact p) {
    __shared__ float sd[BT_MAXB];
    __shared__ int si[BT_MAXB];
    __shared__ BtState<int> st;
    const int nf = p.n_flag[0];
    if (nf <= 0) return;
    const int* qlist = p.n_flag + 1;
    const int B = bt_cap(p.k);
    const int64_t per = (int64_t)p.np * p.C * p.k;
    for (int f = blockIdx.x; f < nf; f += gridDim.x) {
        bt_init(&st);
        for (int64_t c0 = 0; c0 < per; c0 += BT_THREADS) {
            const int64_t c = (int64_t)f * per + c0 + threadIdx.x;
            const bool in = c0 + threadIdx.x < per;
            const int ii = in ? p.ci[c] : -1;
            bt_round(sd, si, &st, p.k, B, ii >= 0 ? p.cd[c] : FX_INF, ii >= 0 ? ii : INT_MAX, ii >= 0);
        }
        bt_flush(sd, si, &st, p.k, B);
        const int64_t q = qlist[f];
        const int c = st.cnt;
        for (int t = threadIdx.x; t < p.k; t += BT_THREADS) {
            const bool valid = t < c;
            p.D[q * p.k + t] = valid ? (METRIC == L2 ? sd[t] : -sd[t]) : (METRIC == L2 ? FLT_MAX : -FLT_MAX);
            p.I[q * p.k + t] = valid ? p.labels[si[t]] : (int64_t)-1;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(IVF_THREADS) void k_ivf_count_bad(const int64_t* __restrict__ coarse, int64_t n,
                                                               int64_t nlist, int* __restrict__ bad) {
    for (int64_t p = (int64_t)blockIdx.x * IVF_THREADS + threadIdx.x; p < n; p += (int64_t)gridDim.x * IVF_THREADS) {
        const int64_t l = coarse[p];
        if (l < 0 || l >= nlist) atomicAdd(bad, 1);
    }
}

__global__ __launch_bounds__(IVF_THREADS) void k_ivf_flag_all(int* __restrict__ flag, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * IVF_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IVF_THREADS) {
        flag[1 + i] = (int)i;
        if (i == 0) flag[0] = (int)n;
    }
}

__global__ void k_ivf_accum(int* __restrict__ total, const int* __restrict__ n_flag) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *total += *n_flag;
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
hipError_t launch_ivf_record(const int64_t* assign, int64_t n, int64_t nlist, int* row_list, unsigned long long* bad,
                             hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ivf_record, dim3(ivf_grid(n, IVF_THREADS)), dim3(IVF_THREADS), 0, s, assign, n, nlist,
                       row_list, bad);
    return hipGetLastError();
}

hipError_t launch_ivf_iota(int64_t* ids, int64_t n, int64_t first, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ivf_iota, dim3(ivf_grid(n, IVF_THREADS)), dim3(IVF_THREADS), 0, s, ids, n, first);
    return hipGetLastError();
}

hipError_t ivf_regroup_bytes(int64_t n, int64_t nlist, size_t* bytes) {
    size_t tb = 0;
    const hipError_t e = ivf_sort_temp(std::max<int64_t>(n, 1), nlist, &tb);
    if (e != hipSuccess) return e;
    *bytes = 2 * ivf_align((size_t)n * 8) + ivf_align(tb);
    return hipSuccess;
}

hipError_t launch_ivf_regroup(const IvfRegroup& r, void* ws, size_t ws_bytes, hipStream_t s) {
    if (r.n <= 0 || r.n > (int64_t)INT32_MAX || r.nlist <= 0 || r.nlist >= (int64_t)INT32_MAX || r.row_bytes % 16 != 0)
        return hipErrorInvalidValue;
    size_t need = 0, tb = 0;
    hipError_t e = ivf_regroup_bytes(r.n, r.nlist, &need);
    if (e == hipSuccess) e = ivf_sort_temp(r.n, r.nlist, &tb);
    if (e != hipSuccess) return e;
    if (!ws || ws_bytes < need) return hipErrorInvalidValue;
    char* base = (char*)ws;
    uint64_t* keys = (uint64_t*)base;
    uint64_t* sorted = (uint64_t*)(base + ivf_align((size_t)r.n * 8));
    void* temp = base + 2 * ivf_align((size_t)r.n * 8);
    hipLaunchKernelGGL(k_ivf_rkeys, dim3(ivf_grid(r.n, IVF_THREADS)), dim3(IVF_THREADS), 0, s, r.row_list, r.n, r.nlist,
                       keys);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = hipcub::DeviceRadixSort::SortKeys(temp, tb, (const uint64_t*)keys, sorted, (int)r.n, IVF_SORT_BEGIN,
                                          32 + ivf_bits(r.nlist), s);
    if (e != hipSuccess) return e;
    if ((e = hipMemsetAsync(r.max_rows, 0, 4, s)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ivf_offsets, dim3(ivf_grid(r.nlist + 1, IVF_THREADS)), dim3(IVF_THREADS), 0, s, sorted,
                       (int)r.n, r.nlist, r.list_off, r.max_rows);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const int cpr = r.row_bytes / 16;
    hipLaunchKernelGGL(k_ivf_gather_codes, dim3(ivf_grid(r.n * cpr, IVF_THREADS)), dim3(IVF_THREADS), 0, s, sorted, r.n,
                       cpr, (const uint4*)r.codes, (uint4*)r.dst_codes);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_ivf_gather_meta, dim3(ivf_grid(r.n, IVF_THREADS)), dim3(IVF_THREADS), 0, s, sorted, r.n,
                       r.norms, r.labels, r.dst_norms, r.dst_labels, r.dst_row_list);
    return hipGetLastError();
}

hipError_t ivf_pairs_temp_bytes(int64_t npairs, int64_t nlist, size_t* bytes) {
    return ivf_sort_temp(std::max<int64_t>(npairs, 1), nlist, bytes);
}

hipError_t launch_ivf_pairs(const IvfPairs& p, void* temp, size_t temp_bytes, hipStream_t s) {
    if (p.npairs <= 0 || p.npairs > (int64_t)INT32_MAX || p.nlist <= 0 || p.nlist >= (int64_t)INT32_MAX)
        return hipErrorInvalidValue;
    // (the caller sized `temp` with ivf_pairs_temp_bytes for this very npairs; hipCUB checks the size it is given)
    if (!temp || temp_bytes == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ivf_pkeys, dim3(ivf_grid(p.npairs, IVF_THREADS)), dim3(IVF_THREADS), 0, s, p.coarse, p.npairs,
                       p.nlist, p.keys, p.bad);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t t1 = temp_bytes;
    e = hipcub::DeviceRadixSort::SortKeys(temp, t1, (const uint64_t*)p.keys, p.sorted, (int)p.npairs, IVF_SORT_BEGIN,
                                          32 + ivf_bits(p.nlist), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ivf_groups, dim3(ivf_grid(p.nlist + 1, IVF_THREADS)), dim3(IVF_THREADS), 0, s, p.sorted,
                       (int)p.npairs, p.nlist, p.list_off, p.seg, p.ngrp);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    t1 = temp_bytes;
    return hipcub::DeviceScan::ExclusiveSum(temp, t1, (const int*)p.ngrp, p.gbase, (int)(p.nlist + 1), s);
}

hipError_t launch_ivf_scan(int st_dt, int metric, const IvfScan& p, hipStream_t s) {
    if (p.row_bytes <= 0 || p.row_bytes % STAGE_B != 0 || p.grid <= 0 || p.grid > (int64_t)INT32_MAX || p.np <= 0 ||
        p.C <= 0 || p.nlist <= 0)
        return hipErrorInvalidValue;
    return dispatch_dt_metric<DT_STORED>(st_dt, metric, [&](auto dt, auto mt) {
        return launch_with_lds(k_ivf_scan<dt(), mt()>, (int)p.grid, SCAN_THREADS, LDS_IVF_BYTES, s, p);
    });
}

hipError_t launch_ivf_exact(int st_dt, int metric, const IvfExact& p, hipStream_t s) {
    if (p.k <= 0 || p.k > FX_BIG_K || p.np <= 0 || p.C <= 0 || !p.labels) return hipErrorInvalidValue;
    hipError_t e = dispatch_dt_metric<DT_STORED>(st_dt, metric, [&](auto dt, auto mt) {
        hipLaunchKernelGGL((k_ivf_exact<dt(), mt()>), dim3(IVF_EXACT_GRID), dim3(BT_THREADS), 0, s, p);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    return launch_ivf_merge(metric, p, s);
}

hipError_t launch_ivf_merge(int metric, const IvfExact& p, hipStream_t s) {
    if (p.k <= 0 || p.k > FX_BIG_K || p.np <= 0 || p.C <= 0 || !p.labels) return hipErrorInvalidValue;
    if (metric == L2) hipLaunchKernelGGL(k_ivf_merge<L2>, dim3(IVF_MERGE_GRID), dim3(BT_THREADS), 0, s, p);
    else hipLaunchKernelGGL(k_ivf_merge<IP>, dim3(IVF_MERGE_GRID), dim3(BT_THREADS), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_ivf_count_bad(const int64_t* coarse, int64_t n, int64_t nlist, int* bad, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ivf_count_bad, dim3(ivf_grid(n, IVF_THREADS)), dim3(IVF_THREADS), 0, s, coarse, n, nlist, bad);
    return hipGetLastError();
}

hipError_t launch_ivf_flag_all(int* flag, int64_t n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ivf_flag_all, dim3(ivf_grid(n, IVF_THREADS)), dim3(IVF_THREADS), 0, s, flag, n);
    return hipGetLastError();
}

hipError_t launch_ivf_accum(int* total, const int* n_flag, hipStream_t s) {
    hipLaunchKernelGGL(k_ivf_accum, dim3(1), dim3(64), 0, s, total, n_flag);
    return hipGetLastError();
}

}  // namespace fx

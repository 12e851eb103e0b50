// fx_select.hip -- filtered search: faiss's IDSelector on the flat index.
//
// faiss: index.search(x, k, params=SearchParameters(sel=IDSelector...)) ranks
// only the rows the selector admits.  Here a selector (FxSelector, fx_host.h)
// is a device image of the admitted subset of an index's rows [0, ntotal):
//
//   row mask     one bit per local row (bit r & 31 of word r >> 5), 4 words
//                per 128-row tile, zero past ntotal;
//   live tiles   the ascending list of the 128-row tiles with a set bit, and
//                its length (SelCounts, read on the device by the scan).
//
//   k_sel_bitmap / k_sel_ids / k_sel_range   build the mask from a faiss
//                IDSelectorBitmap byte string (at any bit offset: ids are
//                row + id_offset), an id array (IDSelectorArray / Batch) or
//                an id range (IDSelectorRange); `invert` (IDSelectorNot) is
//                the complement within the index's rows.
//   k_sel_tiles  one workgroup walks the tiles in order: a block-wide prefix
//                sum of the "tile has a set bit" flags places each live tile,
//                so the list is ascending and the same on every run.
//   k_scan_topk_sel   k_scan_topk's LDS lists and flush over the live tiles
//                only (scan_tiles_128<.., LIVE>), pushing a row only when its
//                mask bit is set.  Rows that are not selected never enter a
//                candidate list, so the refine, the certification (which
//                reasons about what the lists dropped), the re-scan (this same
//                kernel) and the exact fallback (k_fb_scan with the mask) all
//                see one and the same subset.
#include "fx_device.h"

namespace fx {

constexpr int SEL_THREADS = 256;
constexpr int SEL_TILES_THREADS = 1024;

// bits of word w that are rows of the index (rows [32 w, 32 w + 32) below ntotal)
__device__ __forceinline__ uint32_t sel_valid_bits(int64_t w, int64_t ntotal) {
    const int64_t left = ntotal - w * 32;
    return left >= 32 ? 0xffffffffu : left <= 0 ? 0u : (1u << (int)left) - 1u;
}

// one thread per mask word: the 32 bitmap bits from bit offset 32 w + id_offset
__global__ __launch_bounds__(SEL_THREADS) void k_sel_bitmap(const uint8_t* __restrict__ bits, int64_t nbytes,
                                                            int64_t id_offset, int64_t ntotal, int invert,
                                                            int64_t nwords, uint32_t* __restrict__ mask) {
    const int64_t w = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (w >= nwords) return;
    const int64_t b0 = w * 32 + id_offset;  // id of the word's bit 0
    const int64_t byte0 = b0 >> 3;
    const int sh = (int)(b0 & 7);
    unsigned long long v = 0ull;  // bytes byte0 .. byte0 + 4: 40 bits, 32 + sh <= 39 used
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int64_t b = byte0 + j;
        if (b < nbytes) v |= (unsigned long long)bits[b] << (8 * j);  // ids >= 8 nbytes: not members
    }
    uint32_t m = (uint32_t)(v >> sh);
    if (invert) m = ~m;
    mask[w] = m & sel_valid_bits(w, ntotal);
}

// one thread per mask word: rows [lo, hi)
__global__ __launch_bounds__(SEL_THREADS) void k_sel_range(int64_t lo, int64_t hi, int64_t ntotal, int invert,
                                                           int64_t nwords, uint32_t* __restrict__ mask) {
    const int64_t w = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (w >= nwords) return;
    const int64_t a = max(lo - w * 32, (int64_t)0), b = min(hi - w * 32, (int64_t)32);
    uint32_t m = 0u;
    if (a < b) {
        const uint32_t upto_b = b >= 32 ? 0xffffffffu : (1u << (int)b) - 1u;
        m = upto_b & ~((1u << (int)a) - 1u);  // (a < b <= 32: a <= 31)
    }
    if (invert) m = ~m;
    mask[w] = m & sel_valid_bits(w, ntotal);
}

// one thread per id, onto a mask k_sel_range filled (none of the rows, or with
// invert all of them): set, or with invert clear, the row's bit
__global__ __launch_bounds__(SEL_THREADS) void k_sel_ids(const int64_t* __restrict__ ids, int64_t n,
                                                         int64_t id_offset, int64_t ntotal, int invert,
                                                         uint32_t* __restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * SEL_THREADS + threadIdx.x;
    if (i >= n) return;
    const int64_t id = ids[i];
    if (id < id_offset) return;
    const int64_t r = id - id_offset;
    if (r >= ntotal) return;  // ids outside the index are ignored
    const uint32_t bit = 1u << (int)(r & 31);
    if (invert) atomicAnd(mask + (r >> 5), ~bit);
    else atomicOr(mask + (r >> 5), bit);
}

// ONE workgroup: tiles in ascending order, SEL_TILES_THREADS at a time; each
// round's live tiles are placed by a block-wide exclusive prefix sum (wave
// ballots, then the waves' totals), so the list is ascending by construction
__global__ __launch_bounds__(SEL_TILES_THREADS) void k_sel_tiles(const uint32_t* __restrict__ mask, int n_ctiles,
                                                                 int* __restrict__ tiles,
                                                                 SelCounts* __restrict__ cnt) {
    constexpr int NW = SEL_TILES_THREADS / 64;
    __shared__ int s_wave[NW];
    __shared__ unsigned long long s_rows;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_rows = 0ull;
    __syncthreads();
    int base = 0;  // live tiles placed so far (the same value in every thread)
    unsigned long long rows = 0ull;
    for (int t0 = 0; t0 < n_ctiles; t0 += SEL_TILES_THREADS) {
        const int t = t0 + tid;
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        if (t < n_ctiles) w = ((const uint4*)mask)[t];  // the tile's 4 words
        const bool live = (w.x | w.y | w.z | w.w) != 0u;
        rows += (unsigned)(__popc(w.x) + __popc(w.y) + __popc(w.z) + __popc(w.w));
        const unsigned long long b = __ballot(live);
        if (lane == 0) s_wave[wave] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int v = 0; v < NW; ++v) {
            const int c = s_wave[v];
            before += v < wave ? c : 0;
            total += c;
        }
        if (live) tiles[base + before + __popcll(b & ((1ull << lane) - 1ull))] = t;
        base += total;
        __syncthreads();  // s_wave is rewritten next round
    }
    if (rows != 0ull) atomicAdd(&s_rows, rows);
    __syncthreads();
    if (tid == 0) {
        cnt->rows = (long long)s_rows;
        cnt->tiles = base;
        cnt->pad = 0;
    }
}

// ---------------------------------------------------------------------------
// the filtered scan: k_scan_topk (fx_kernels.hip) over the live tiles, rows
// gated by their mask bit
// ---------------------------------------------------------------------------
template <int DT, int METRIC>
__global__ __launch_bounds__(SCAN_THREADS, 1) void k_scan_topk_sel(ScanParams p, const uint32_t* __restrict__ mask,
                                                                   const int* __restrict__ tiles,
                                                                   const SelCounts* __restrict__ selcnt) {
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int qtile, split;
    map_block(blockIdx.x, p, qtile, split);
    const int64_t nq = p.nq_dev ? min((int64_t)*p.nq_dev, p.nq) : p.nq;
    if (qtile >= p.n_qtiles || split >= p.splits || (int64_t)qtile * TILE_Q >= nq) return;
    const int64_t q0 = (int64_t)qtile * TILE_Q;

    float* lst_d = (float*)(smem + LDS_LD_OFF);
    int* lst_i = (int*)(smem + LDS_LI_OFF);
    int* cnt = (int*)(smem + LDS_CNT_OFF);
    float* tau = (float*)(smem + LDS_TAU_OFF);
    volatile int* flag = (volatile int*)(smem + LDS_FLAG_OFF);

    for (int x = tid; x < TILE_Q; x += SCAN_THREADS) { cnt[x] = 0; tau[x] = FX_INF; }
    if (tid == 0) *flag = 0;

    // per finished live tile: filter against the mask and tau, push into the LDS lists (always_inline: see
    // k_scan_topk).  A wave's 64 rows of the tile are two mask words, fetched wave-uniformly.
    scan_tiles_128<DT, METRIC, true>(
        p, smem, qtile, split,
        [&](const auto& acc, const auto& yn, int trow0, int rlim, int rl0) __attribute__((always_inline)) {
            const uint32_t* mw = mask + (trow0 >> 5) + (wave >> 1) * 2;  // rows trow0 + 64 wm ..
            const uint32_t w0 = __builtin_amdgcn_readfirstlane(mw[0]);
            const uint32_t w1 = __builtin_amdgcn_readfirstlane(mw[1]);
            // selected rows of this lane: bit m * 4 + i for local row rl0 + 16 m + i
            // (rl0 = 64 wm + 4 (lane >> 4): rows of m = 0, 1 in w0, of m = 2, 3 in w1)
            const int sh = 4 * (lane >> 4);
            unsigned sel = 0u;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const uint32_t w = m < 2 ? w0 : w1;
                sel |= ((w >> (sh + (m & 1) * 16)) & 0xfu) << (m * 4);
            }
            int qloc[4];
            bool qv[4];
            float tn[4];
            unsigned pend[4];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                qloc[n] = tile_qloc(n);
                qv[n] = q0 + qloc[n] < nq;
                tn[n] = tau[qloc[n]];
                pend[n] = 0u;
            }
            int ovf = 0;
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float v = METRIC == L2 ? acc[m][n][i] + yn[m][i] : acc[m][n][i];
                        const int rl = tile_rloc(rl0, m, i);
                        if (qv[n] && ((sel >> (m * 4 + i)) & 1u) && rl < rlim && v <= tn[n]) {
                            const int s = atomicAdd(&cnt[qloc[n]], 1);
                            if (s < CAP) {
                                lst_d[qloc[n] * CAP + s] = v;
                                lst_i[qloc[n] * CAP + s] = trow0 + rl;
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
                                        lst_i[qloc[n] * CAP + s] = trow0 + tile_rloc(rl0, m, i);
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
        },
        tiles, &selcnt->tiles);

    // final flush: sorted top-KP per query of this (query tile, split) -- also of a split that got no
    // live tile (empty lists: id -1, key +inf), since the refine reads every split
    __syncthreads();
    const int64_t obase = ((int64_t)qtile * p.splits + split) * TILE_Q;
    for (int q = wave; q < TILE_Q; q += 4) {
        if (q0 + q >= nq) break;
        const int c = min(cnt[q], CAP);
        float d = lane < c ? lst_d[q * CAP + lane] : FX_INF;
        int i = lane < c ? lst_i[q * CAP + lane] : INT_MAX;
        sort64(d, i, lane);
        if (lane < KP) {
            p.cand_d[(obase + q) * KP + lane] = d;
            p.cand_i[(obase + q) * KP + lane] = i == INT_MAX ? -1 : i;
        }
    }
}

namespace {

unsigned sel_blocks(int64_t items) { return (unsigned)std::max<int64_t>(1, (items + SEL_THREADS - 1) / SEL_THREADS); }

}  // namespace

hipError_t launch_sel_bitmap(const uint8_t* bits, int64_t nbytes, int64_t id_offset, int64_t ntotal, int invert,
                             uint32_t* mask, hipStream_t s) {
    const int64_t nw = sel_mask_words(ntotal);
    if (nw <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sel_bitmap, dim3(sel_blocks(nw)), dim3(SEL_THREADS), 0, s, bits, nbytes, id_offset, ntotal,
                       invert, nw, mask);
    return hipGetLastError();
}

hipError_t launch_sel_range(int64_t lo, int64_t hi, int64_t ntotal, int invert, uint32_t* mask, hipStream_t s) {
    const int64_t nw = sel_mask_words(ntotal);
    if (nw <= 0) return hipSuccess;
    if (lo < 0 || hi < lo || hi > ntotal) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sel_range, dim3(sel_blocks(nw)), dim3(SEL_THREADS), 0, s, lo, hi, ntotal, invert, nw, mask);
    return hipGetLastError();
}

hipError_t launch_sel_ids(const int64_t* ids, int64_t n, int64_t id_offset, int64_t ntotal, int invert,
                          uint32_t* mask, hipStream_t s) {
    // no row (invert: every row), then one atomic per id
    hipError_t e = launch_sel_range(0, 0, ntotal, invert, mask, s);
    if (e != hipSuccess || n <= 0 || ntotal <= 0) return e;
    hipLaunchKernelGGL(k_sel_ids, dim3(sel_blocks(n)), dim3(SEL_THREADS), 0, s, ids, n, id_offset, ntotal, invert,
                       mask);
    return hipGetLastError();
}

hipError_t launch_sel_tiles(const uint32_t* mask, int64_t ntotal, int* tiles, SelCounts* cnt, hipStream_t s) {
    const int n_ctiles = (int)((ntotal + TILE_R - 1) / TILE_R);
    hipLaunchKernelGGL(k_sel_tiles, dim3(1), dim3(SEL_TILES_THREADS), 0, s, mask, n_ctiles, tiles, cnt);
    return hipGetLastError();
}

hipError_t launch_scan_sel(int st_dt, int metric, const ScanParams& p, const uint32_t* mask, const int* tiles,
                           const SelCounts* cnt, hipStream_t s) {
    if (p.row_bytes <= 0 || p.row_bytes % STAGE_B != 0 || p.grid <= 0 || p.qt != TILE_Q || p.tr != TILE_R || !mask ||
        !tiles || !cnt)
        return hipErrorInvalidValue;
    return dispatch_dt_metric<DT_STORED>(st_dt, metric, [&](auto dt, auto mt) {
        return launch_with_lds(k_scan_topk_sel<dt(), mt()>, p.grid, SCAN_THREADS, LDS_SCAN_BYTES, s, p, mask, tiles,
                               cnt);
    });
}

}  // namespace fx

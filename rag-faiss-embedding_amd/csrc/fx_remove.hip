// fx_remove.hip -- remove_ids: in-place compaction of the stored rows.
//
// faiss: IndexFlatCodes::remove_ids(sel) drops the selected rows; the kept
// rows keep their order and are renumbered densely.  Here the selector's row
// mask (fx_select.hip: a set bit = selected = REMOVED) drives a compaction of
// `codes` and `norms` where they lie.  Every destination row is at or below
// its source row, so a workgroup writing row j could destroy a source row
// that another has not read yet.  The order comes from the stream, never from
// workgroups waiting on each other: the host (fx_api_remove.cpp remove_rows) cuts
// the rows from the first removed one upward into ascending chunks of source
// rows, one k_move_rows launch each, and a launch only ever writes
//   - below the first source row of its chunk (a "direct" chunk: its
//     destination range ends at or before its source range begins), or
//   - into the staging buffer, which one device-to-device copy then puts in
//     place (the destination never extends past the chunk's own source range,
//     so the sources of later chunks are intact).
//
//   k_keep_count / k_keep_blk_scan / k_keep_prefix   per 32-row mask word, the
//                number of kept rows before it (a two-level exclusive scan:
//                block sums, one workgroup scanning them, the words of each
//                block), that count at every 1024-row boundary for the host's
//                plan, the first removed row and the kept total.
//   k_move_rows  one wave per mask word of the chunk: the word's kept rows go
//                to consecutive destination rows, so the wave writes ONE
//                contiguous run of 16-byte units and reads each kept row's
//                units in order; four units per lane in flight.  The same wave
//                moves the rows' norms.
//   k_norm_max   max_sq_bits <- max over norms[0, n) (zeroed by the host
//                first), as launch_convert_rows maintains it.
#include "fx_device.h"

#include <algorithm>

namespace fx {

constexpr int RM_THREADS = RM_WORDS_PER_BLOCK;  // one thread per mask word
constexpr int RM_SCAN_THREADS = 1024;
constexpr int RM_MOVE_GRID = 2048;  // workgroups of k_move_rows at most (4 words each per round)

// rows of word w below ntotal, as bits
__device__ __forceinline__ uint32_t rm_valid_bits(int64_t w, int64_t ntotal) {
    const int64_t left = ntotal - w * 32;
    return left >= 32 ? 0xffffffffu : left <= 0 ? 0u : (1u << (int)left) - 1u;
}

// sum of v over the workgroup's RM_THREADS threads -> every thread; *excl: the
// sum over the threads before this one
__device__ __forceinline__ unsigned rm_block_scan(unsigned v, unsigned* excl, unsigned* s_wave) {
    constexpr int NW = RM_THREADS / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    unsigned before = 0u, total = 0u;
#pragma unroll
    for (int x = 0; x < NW; ++x) {
        const unsigned c = s_wave[x];
        before += x < wave ? c : 0u;
        total += c;
    }
    __syncthreads();  // (s_wave may be rewritten by the caller's next round)
    *excl = before + inc - v;
    return total;
}

// bsum[b] <- kept rows of the block's RM_THREADS words; info[0] <- min over the removed rows (atomicMin)
__global__ __launch_bounds__(RM_THREADS) void k_keep_count(const uint32_t* __restrict__ mask, int64_t ntotal,
                                                           int64_t nwords, unsigned* __restrict__ bsum,
                                                           unsigned* __restrict__ info) {
    __shared__ unsigned s_wave[RM_THREADS / 64];
    const int64_t w = (int64_t)blockIdx.x * RM_THREADS + threadIdx.x;
    uint32_t keep = 0u, gone = 0u;
    if (w < nwords) {
        const uint32_t valid = rm_valid_bits(w, ntotal), m = mask[w];
        keep = ~m & valid;
        gone = m & valid;
    }
    unsigned first = gone ? (unsigned)(w * 32 + (__ffs(gone) - 1)) : 0xffffffffu;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) first = min(first, (unsigned)__shfl_xor(first, d));
    if ((threadIdx.x & 63) == 0 && first != 0xffffffffu) atomicMin(info, first);
    unsigned excl;
    const unsigned total = rm_block_scan((unsigned)__popc(keep), &excl, s_wave);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// ONE workgroup: bsum[0, nblk) <- its exclusive prefix sums, in place; info[1] <- the total
__global__ __launch_bounds__(RM_SCAN_THREADS) void k_keep_blk_scan(unsigned* __restrict__ bsum, int nblk,
                                                                   unsigned* __restrict__ info) {
    constexpr int NW = RM_SCAN_THREADS / 64;
    __shared__ unsigned s_wave[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned base = 0u;  // the same value in every thread
    for (int b0 = 0; b0 < nblk; b0 += RM_SCAN_THREADS) {
        const int b = b0 + tid;
        const unsigned v = b < nblk ? bsum[b] : 0u;
        unsigned inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned o = __shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        unsigned before = 0u, total = 0u;
#pragma unroll
        for (int x = 0; x < NW; ++x) {
            const unsigned c = s_wave[x];
            before += x < wave ? c : 0u;
            total += c;
        }
        if (b < nblk) bsum[b] = base + before + inc - v;
        base += total;
        __syncthreads();  // s_wave is rewritten next round
    }
    if (tid == 0) info[1] = base;
}

// prefix[w] <- kept rows before word w; gp[w / 32] <- the same at every 32nd word (1024-row boundaries)
__global__ __launch_bounds__(RM_THREADS) void k_keep_prefix(const uint32_t* __restrict__ mask, int64_t ntotal,
                                                            int64_t nwords, const unsigned* __restrict__ boff,
                                                            unsigned* __restrict__ prefix, unsigned* __restrict__ gp) {
    __shared__ unsigned s_wave[RM_THREADS / 64];
    const int64_t w = (int64_t)blockIdx.x * RM_THREADS + threadIdx.x;
    const uint32_t keep = w < nwords ? ~mask[w] & rm_valid_bits(w, ntotal) : 0u;
    unsigned excl;
    (void)rm_block_scan((unsigned)__popc(keep), &excl, s_wave);
    if (w < nwords) {
        const unsigned p = boff[blockIdx.x] + excl;
        prefix[w] = p;
        if ((w & 31) == 0) gp[w >> 5] = p;
    }
}

// position of the n-th (from 0) set bit of m; n < popc(m)
__host__ __device__ __forceinline__ int rm_nth_bit(uint32_t m, int n) {
    int pos = 0;
#pragma unroll
    for (int sh = 16; sh >= 1; sh >>= 1) {
        const uint32_t lo = (m >> pos) & ((1u << sh) - 1u);
#if defined(__HIP_DEVICE_COMPILE__)
        const int c = __popc(lo);
#else
        const int c = __builtin_popcount(lo);
#endif
        if (n >= c) {
            n -= c;
            pos += sh;
        }
    }
    return pos;
}

struct MoveParams {
    const char* codes;       // source rows (the index's own)
    const float* norms;
    const uint32_t* mask;    // set bit: the row is removed
    const unsigned* prefix;  // kept rows before each mask word
    int64_t ntotal;
    int64_t s0, s1;          // source rows [s0, s1) of this chunk
    int units;               // 16-byte units per row (row_bytes / 16)
    char* dst_codes;         // kept row r -> row prefix(r) - dbase of dst_codes / dst_norms
    float* dst_norms;
    int64_t dbase;
};

// One wave per mask word of [s0, s1), round-robin over the grid's waves.
__global__ __launch_bounds__(RM_THREADS) void k_move_rows(MoveParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t w0 = p.s0 >> 5, w1 = (p.s1 + 31) >> 5;  // words touching the chunk
    const int64_t nwaves = (int64_t)gridDim.x * (RM_THREADS / 64);
    const unsigned V = (unsigned)p.units;
    for (int64_t w = w0 + (int64_t)blockIdx.x * (RM_THREADS / 64) + (threadIdx.x >> 6); w < w1; w += nwaves) {
        const uint32_t keep_all = ~p.mask[w] & rm_valid_bits(w, p.ntotal);
        // the word's bits inside [s0, s1)
        const int64_t a = max(p.s0 - w * 32, (int64_t)0), b = min(p.s1 - w * 32, (int64_t)32);
        const uint32_t upto_b = b >= 32 ? 0xffffffffu : (1u << (int)b) - 1u;
        const uint32_t below_a = (1u << (int)a) - 1u;  // (a <= 31: the word touches the chunk)
        const uint32_t keep = keep_all & upto_b & ~below_a;
        if (keep == 0u) continue;
        // destination row of the word's first kept row of the chunk
        const int64_t drow = (int64_t)p.prefix[w] + __popc(keep_all & below_a) - p.dbase;
        const int nkept = __popc(keep);
        if (lane < 32 && ((keep >> lane) & 1u))
            p.dst_norms[drow + __popc(keep & ((1u << lane) - 1u))] = p.norms[w * 32 + lane];
        const uint4* src = (const uint4*)p.codes + w * 32 * (int64_t)V;
        uint4* dst = (uint4*)p.dst_codes + drow * (int64_t)V;
        const unsigned total = (unsigned)nkept * V;  // <= 32 * 2^27 / 16 units: fits
        for (unsigned u0 = 0; u0 < total; u0 += 256u) {
            uint4 v[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned u = u0 + 64u * i + lane;
                if (u < total) {
                    const unsigned j = u / V, o = u - j * V;
                    v[i] = src[(int64_t)rm_nth_bit(keep, (int)j) * V + o];
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const unsigned u = u0 + 64u * i + lane;
                if (u < total) dst[u] = v[i];
            }
        }
    }
}

// bits[0] <- max(bits[0], max of norms[0, n) as float bits): non-negative floats (and +inf) order as uints
__global__ __launch_bounds__(RM_THREADS) void k_norm_max(const float* __restrict__ norms, int64_t n,
                                                         unsigned* __restrict__ bits) {
    unsigned m = 0u;
    for (int64_t i = (int64_t)blockIdx.x * RM_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * RM_THREADS)
        m = max(m, __float_as_uint(norms[i]));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (unsigned)__shfl_xor(m, d));
    if ((threadIdx.x & 63) == 0 && m != 0u) atomicMax(bits, m);
}

hipError_t launch_keep_prefix(const uint32_t* mask, int64_t ntotal, unsigned* prefix, unsigned* gp, unsigned* bsum,
                              unsigned* info, hipStream_t s) {
    const int64_t nw = sel_mask_words(ntotal);
    if (nw <= 0 || !mask || !prefix || !gp || !bsum || !info) return hipErrorInvalidValue;
    const int64_t nblk = rm_prefix_blocks(ntotal);
    hipError_t e = hipMemsetAsync(info, 0xff, 4, s);  // no removed row yet
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_keep_count, dim3((unsigned)nblk), dim3(RM_THREADS), 0, s, mask, ntotal, nw, bsum, info);
    hipLaunchKernelGGL(k_keep_blk_scan, dim3(1), dim3(RM_SCAN_THREADS), 0, s, bsum, (int)nblk, info);
    hipLaunchKernelGGL(k_keep_prefix, dim3((unsigned)nblk), dim3(RM_THREADS), 0, s, mask, ntotal, nw,
                       (const unsigned*)bsum, prefix, gp);
    return hipGetLastError();
}

hipError_t launch_move_rows(const char* codes, const float* norms, const uint32_t* mask, const unsigned* prefix,
                            int64_t ntotal, int row_bytes, int64_t s0, int64_t s1, char* dst_codes, float* dst_norms,
                            int64_t dbase, hipStream_t s) {
    if (row_bytes <= 0 || row_bytes % ROW_ALIGN != 0 || s0 < 0 || s1 > ntotal || !codes || !norms || !mask ||
        !prefix || !dst_codes || !dst_norms)
        return hipErrorInvalidValue;
    if (s0 >= s1) return hipSuccess;
    MoveParams p;
    p.codes = codes;
    p.norms = norms;
    p.mask = mask;
    p.prefix = prefix;
    p.ntotal = ntotal;
    p.s0 = s0;
    p.s1 = s1;
    p.units = row_bytes / 16;
    p.dst_codes = dst_codes;
    p.dst_norms = dst_norms;
    p.dbase = dbase;
    const int64_t words = ((s1 + 31) >> 5) - (s0 >> 5);
    const int64_t blocks = (words + RM_THREADS / 64 - 1) / (RM_THREADS / 64);
    hipLaunchKernelGGL(k_move_rows, dim3((unsigned)std::min<int64_t>(blocks, RM_MOVE_GRID)), dim3(RM_THREADS), 0, s,
                       p);
    return hipGetLastError();
}

hipError_t launch_norm_max(const float* norms, int64_t n, unsigned* bits, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const int64_t blocks = (n + RM_THREADS - 1) / RM_THREADS;
    hipLaunchKernelGGL(k_norm_max, dim3((unsigned)std::min<int64_t>(blocks, 1024)), dim3(RM_THREADS), 0, s, norms, n,
                       bits);
    return hipGetLastError();
}

}  // namespace fx

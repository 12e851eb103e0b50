// fx_pq.hip -- product quantizer: faiss's IndexPQ with 8-bit codes, restated from
// memory and not checked against a faiss build (include/fx_index.h "product
// quantizer").
//
// A row is M code bytes (stride roundup(M, 16), padding 0): byte m names one of
// the 256 fp32 centroids of sub-quantizer m, and the row decodes to their
// concatenation -- a gather, no arithmetic.  A search ranks the DECODED rows
// exactly, as the flat index ranks its stored rows.
//
//   k_pq_encode  code[row][m] = argmin_j of the fp64 squared distance between the
//                subvector and centroid j (dimensions ascending, every operation
//                rounded once, the lowest j on a tie).
//   k_pq_ny      the row constant n_y = |decode|^2 (fp64 sum in dimension order,
//                rounded once).
//   k_pq_decode  the codec's other direction (sa_decode, reconstruct*).
//   k_pq_prep    per query the [hi | lo] bf16 planes of x' = -2 x (IP: -x), the
//                shift |x|^2 (IP: 0) and the bound E.
//   k_pq_scan    a sibling of scan_tiles_128 + k_scan_topk's epilogue whose A
//                operand is not read from the rows but gathered from the
//                codebook's scan image: a stage is 32 dimensions, a lane's 16-B
//                piece is 8 dimensions of one centroid, and the lane points its
//                LDS-DMA at plane[m][code[row][m]].  Three bf16 MFMAs per block
//                and k-chunk (hi.hi, hi.lo, lo.hi) into one fp32 accumulator set.
//   k_pq_refine  k_sq_refine with the exact recomputation gathering the
//                candidate's fp32 centroids.
//   k_pq_exact / k_pq_merge   the exact path: fp64 distances of every decoded
//                row.  Serves the flagged queries, KP < k <= FX_BIG_K and every
//                index with dsub % 8 != 0: correct, but slow.
#include "fx_sq_common.h"

#include <algorithm>

namespace fx {

namespace {

constexpr int PQ_THREADS = 256;
constexpr int PQ_GRID_CAP = 4096;

unsigned pq_grid(int64_t items, int per_block) {
    const int64_t g = (items + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : g > PQ_GRID_CAP ? PQ_GRID_CAP : g);
}

}  // namespace

// ---------------------------------------------------------------------------
// encode / decode
// ---------------------------------------------------------------------------
// one thread per (row, sub-quantizer); blockIdx.y = m, so a wave reads every
// centroid value as one broadcast.  DS = dsub when it is 8 (the subvector stays
// in registers), else 0.
template <int DS>
__global__ __launch_bounds__(PQ_THREADS) void k_pq_encode(const void* __restrict__ x, int x_dt, int64_t n, int d,
                                                          int dsub, const float* __restrict__ cb,
                                                          uint8_t* __restrict__ out, int stride) {
#pragma clang fp contract(off)
    const int m = blockIdx.y;
    const float* cm = cb + (int64_t)m * PQ_KSUB * dsub;
    for (int64_t r = (int64_t)blockIdx.x * PQ_THREADS + threadIdx.x; r < n; r += (int64_t)gridDim.x * PQ_THREADS) {
        const int64_t x0 = r * d + (int64_t)m * dsub;
        double xs[DS > 0 ? DS : 1];
        if (DS > 0) {
#pragma unroll
            for (int e = 0; e < DS; ++e) xs[e] = (double)load_elem(x, x0 + e, x_dt);
        }
        double best = 0.0;
        int bj = 0;
        for (int j = 0; j < PQ_KSUB; ++j) {
            const float* c = cm + j * dsub;
            double acc = 0.0;
            if (DS > 0) {
#pragma unroll
                for (int e = 0; e < DS; ++e) {
                    const double df = xs[e] - (double)c[e];
                    const double sq = df * df;
                    acc = acc + sq;
                }
            } else {
                for (int e = 0; e < dsub; ++e) {
                    const double df = (double)load_elem(x, x0 + e, x_dt) - (double)c[e];
                    const double sq = df * df;
                    acc = acc + sq;
                }
            }
            if (j == 0 || acc < best) {  // (a NaN distance never wins: code 0)
                best = acc;
                bj = j;
            }
        }
        out[r * stride + m] = (uint8_t)bj;
    }
}

// one thread per row: the fp64 sum in dimension order (every square of an fp32
// value is exact in fp64, so each step is one rounding)
__global__ __launch_bounds__(PQ_THREADS) void k_pq_ny(const uint8_t* __restrict__ codes, int stride, int64_t n, int M,
                                                      int dsub, const float* __restrict__ cb, float* __restrict__ ny) {
#pragma clang fp contract(off)
    for (int64_t r = (int64_t)blockIdx.x * PQ_THREADS + threadIdx.x; r < n; r += (int64_t)gridDim.x * PQ_THREADS) {
        double acc = 0.0;
        for (int m = 0; m < M; ++m) {
            const float* c = cb + ((int64_t)m * PQ_KSUB + codes[r * stride + m]) * dsub;
            for (int e = 0; e < dsub; ++e) {
                const double y = (double)c[e];
                const double sq = y * y;
                acc = acc + sq;
            }
        }
        ny[r] = (float)acc;
    }
}

__global__ __launch_bounds__(PQ_THREADS) void k_pq_decode(const uint8_t* __restrict__ codes, int stride, int64_t nrows,
                                                          const int64_t* __restrict__ keys, int64_t key0, int64_t n,
                                                          int M, int dsub, const float* __restrict__ cb,
                                                          float* __restrict__ out) {
    const int d = M * dsub;
    const int64_t items = n * d;
    for (int64_t e = (int64_t)blockIdx.x * PQ_THREADS + threadIdx.x; e < items; e += (int64_t)gridDim.x * PQ_THREADS) {
        const int64_t i = e / d;
        const int j = (int)(e - i * d);
        const int m = j / dsub;
        const int64_t r = keys ? keys[i] : key0 + i;
        float v = __uint_as_float(0xffffffffu);
        if (r >= 0 && r < nrows) v = cb[((int64_t)m * PQ_KSUB + codes[r * stride + m]) * dsub + (j - m * dsub)];
        out[e] = v;
    }
}

// ---------------------------------------------------------------------------
// query preparation: one wave per query row of the padded batch.
//
// With x' = -2 x (IP: -x; exact scalings), x'_hi = rn_bf16(x'), x'_lo =
// rn_bf16(x' - x'_hi) and the same split of every centroid value, the scan sums
//   S = x'_hi.y_hi + x'_hi.y_lo + x'_lo.y_hi  =  x'.y - x'.r_y - r_x.y + r_x.r_y - x'_lo.y_lo
// (r_x = x' - x'_hi - x'_lo, r_y = y - y_hi - y_lo; bf16 products are exact in
// fp32) and its key is fl(n_y) + fl(S) (IP: fl(S)); key + shift estimates the
// exact key |x - y|^2 (IP: -x.y) of the decoded fp32 row y:
//   |key + shift - exact| <= E =   |x'| Ry                 the codebook residual
//                                + |r_x| (Y + Ry)          the query residual
//                                + |x'_lo| Yl              the dropped lo.lo product
//                                + gamma_{3K+1} 1.03 |x'| Y   the fp32 accumulation of the 3 K products
//                                + u (Y^2 + 1.03 |x'| Y)      the key's last addition      (L2: Y^2 terms)
//                                + u Y^2                      the rounding of n_y
// Y = max |decode|, Ry = max |r_y|, Yl = max |y_lo| over every code row: square
// roots of sums over m of per-sub-quantizer maxima (fx_api_pq.cpp), so they
// hold for any row whatever its codes.  1.03 covers |x'_hi| <= (1 + 2^-8) |x'|
// and the two cross products' 2^-8 each.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(PQ_THREADS) void k_pq_prep(PqPrep p, double gamma) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= p.nq_pad) return;
    if (r == 0 && lane == 0)
        for (int i = 0; i < 2; ++i)
            if (p.zero[i]) *p.zero[i] = 0;
    const bool live = r < p.nq;
    const int kp = p.kp, d = p.d;
    const bool l2 = p.metric == L2;
    const float scale = l2 ? -2.0f : -1.0f;
    uint16_t* hi_row = p.planes + r * (int64_t)kp;
    uint16_t* lo_row = p.planes + (p.nq_pad + r) * (int64_t)kp;
    double xx = 0.0, rr = 0.0, ll = 0.0;
    for (int c = lane; c < kp; c += 64) {
        const float v = (live && c < d) ? load_elem(p.q, r * d + c, p.q_dt) : 0.0f;
        p.qf32[r * (int64_t)kp + c] = v;
        const float xs = v == 0.0f ? 0.0f : scale * v;  // (padding and zeros as +0, not -0)
        const bool fin = __builtin_isfinite(xs);
        const uint16_t h = f2bf(xs);
        const float hf = bf2f(h);
        const float rest = xs - hf;  // exact in fp32: hi is within 2^-8 |x'| of x'
        const uint16_t l = fin ? f2bf(rest) : (uint16_t)0;
        const double res = (double)rest - (double)bf2f(l);
        hi_row[c] = fin ? h : (uint16_t)0;
        lo_row[c] = l;
        xx += (double)v * (double)v;
        rr += res * res;
        ll += (double)bf2f(l) * (double)bf2f(l);
    }
    xx = wave_sum_f64(xx);
    rr = wave_sum_f64(rr);
    ll = wave_sum_f64(ll);
    if (lane != 0 || !live) return;
    const bool bad = !(xx < 1e300);  // (a non-finite query: never certified)
    const double u = 5.9604644775390625e-8;  // 2^-24
    const double xn = (l2 ? 2.0 : 1.0) * sqrt(xx);  // |x'|
    const double A = 1.03 * xn * p.Y;
    double eps = xn * p.Ry + sqrt(rr) * (p.Y + p.Ry) + sqrt(ll) * p.Yl + (gamma + u) * A;
    if (l2) eps += 2.0 * u * p.Y * p.Y;
    const double sh = l2 ? xx : 0.0;
    eps += 1e-12 * sh;
    p.qeps[r] = bad ? FX_INF : (float)(eps * 1.0625 + 1e-30);
    p.qrho[r] = (float)(sqrt(rr) * 1.0000002);
    p.qshift[r] = sh;
}

// ---------------------------------------------------------------------------
// the scan.  Per 32-dimension stage the workgroup moves 32 one-KiB pieces: the
// hi and lo blocks of 8 row blocks (A) and of 8 query blocks (B), 4 + 4 per
// wave.  An A piece is 16 rows x 64 B: lane l stages row l & 15, dimensions 32 ks
// + 8 (l >> 4) .. + 7, which are 8 dimensions of centroid code[row][m] of sub-
// quantizer m = (4 ks + (l >> 4)) / (dsub / 8): the lane's LDS-DMA source is that
// piece of the scan image, and the same address + plane_bytes for the lo block.
// Pieces at or past d (the last stage of a d that is no multiple of 32) gather
// the image's zero piece.  Every gather address is image + (m * 256 + code) *
// dsub * 2 + piece with m < M and code a byte, so it lies inside the image
// whatever the code bytes hold; the bytes themselves are read at rows below
// n_ctiles * 128 <= the allocation (padding rows hold code 0).
//
// The code bytes feed a dependent address, so the bytes of stage g + 2 are
// loaded into registers before stage g + 1 is issued: the stage's DMAs never
// wait for them.  Ordering as the plain loops: vmcnt(0) + s_barrier per stage,
// a buffer read one phase after the wait that retires it, no swizzle.
// ---------------------------------------------------------------------------
template <int METRIC>
__global__ __launch_bounds__(SCAN_THREADS, 1) void k_pq_scan(PqScan p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int qtile = (int)(blockIdx.x % (unsigned)p.n_qtiles), split = (int)(blockIdx.x / (unsigned)p.n_qtiles);
    if (split >= p.splits) return;
    const int64_t q0 = (int64_t)qtile * TILE_Q;

    float* lst_d = (float*)(smem + LDS_LD_OFF);
    int* lst_i = (int*)(smem + LDS_LI_OFF);
    int* cnt = (int*)(smem + LDS_CNT_OFF);
    float* tau = (float*)(smem + LDS_TAU_OFF);
    volatile int* flag = (volatile int*)(smem + LDS_FLAG_OFF);

    for (int x = tid; x < TILE_Q; x += SCAN_THREADS) { cnt[x] = 0; tau[x] = FX_INF; }
    if (tid == 0) *flag = 0;

    const int ct0 = (int)((int64_t)split * p.n_ctiles / p.splits);
    const int ct1 = (int)((int64_t)(split + 1) * p.n_ctiles / p.splits);
    const int kp = p.kp;
    const int nks = kp / PQ_STAGE_D;
    const int G = (ct1 - ct0) * nks;
    const int s8 = p.dsub >> 3;   // 16-B pieces per centroid
    const int npc = p.d >> 3;     // pieces of a row that hold dimensions
    const int lgrp = lane >> 4;
    const int64_t zoff = p.plane_bytes - 16;  // the zero piece
    const int cmul = p.dsub * 2;              // bytes from one centroid to the next

    int lrow[2];
    int64_t boff[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        lrow[j] = (wave * 2 + j) * 16 + (lane & 15);
        boff[j] = ((q0 + lrow[j]) * kp + lgrp * 8) * 2;
    }
    const char* bplanes = (const char*)p.planes;
    const int64_t bplane = p.nq_pad * (int64_t)kp * 2;

    // what a lane needs to form its two gather addresses of one stage
    struct Gather {
        int64_t base;   // byte offset of centroid 0's piece in a plane (the zero piece: past d)
        int mul;        // cmul, or 0 past d
        unsigned c[2];  // the two rows' code bytes
    };
    auto fetch = [&](int g) -> Gather {
        const int t = g / nks, ks = g - t * nks;
        const int pi = ks * 4 + lgrp;
        const bool has = pi < npc;
        const int m = has ? pi / s8 : 0;
        const int o8 = has ? pi - m * s8 : 0;
        Gather x;
        x.base = has ? ((int64_t)m * PQ_KSUB * p.dsub + o8 * 8) * 2 : zoff;
        x.mul = has ? cmul : 0;
        const uint8_t* cr = p.codes + (int64_t)(ct0 + t) * TILE_R * p.stride + m;
#pragma unroll
        for (int j = 0; j < 2; ++j) x.c[j] = cr[(int64_t)lrow[j] * p.stride];
        return x;
    };
    auto issue = [&](int g, const Gather& x) {
        const int t = g / nks, ks = g - t * nks;
        char* buf = smem + (g & 1) * PQ_STAGE_BYTES;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int blk = (wave * 2 + j) * 1024;
            const char* a = p.img + x.base + (int64_t)(x.c[j] & 0xffu) * x.mul;
            const char* b = bplanes + boff[j] + ks * (PQ_STAGE_D * 2);
            glds16(a, buf + blk);
            glds16(a + p.plane_bytes, buf + 8192 + blk);
            glds16(b, buf + 16384 + blk);
            glds16(b + bplane, buf + 24576 + blk);
        }
        if (METRIC == L2 && ks == 0 && wave == 0 && lane < 32)
            glds16(p.ny + (int64_t)(ct0 + t) * TILE_R + lane * 4, smem + LDS_NORM_OFF + (t & 1) * (TILE_R * 4));
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};

    Gather nxt{};
    if (G > 0) {
        const Gather first = fetch(0);
        if (G > 1) nxt = fetch(1);
        issue(0, first);
    }
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");

    int t = 0, ks = 0;
    for (int g = 0; g < G; ++g) {
        Gather after{};
        if (g + 2 < G) after = fetch(g + 2);
        if (g + 1 < G) issue(g + 1, nxt);
        nxt = after;
        const char* buf = smem + (g & 1) * PQ_STAGE_BYTES;
        bf16x8 ah[4], al[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            ah[m] = *(const bf16x8*)(buf + (wm * 4 + m) * 1024 + lane * 16);
            al[m] = *(const bf16x8*)(buf + 8192 + (wm * 4 + m) * 1024 + lane * 16);
        }
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            const bf16x8 bh = *(const bf16x8*)(buf + 16384 + (wn * 4 + n) * 1024 + lane * 16);
            const bf16x8 bl = *(const bf16x8*)(buf + 24576 + (wn * 4 + n) * 1024 + lane * 16);
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[m], bh, acc[m][n], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[m], bl, acc[m][n], 0, 0, 0);
#pragma unroll
            for (int m = 0; m < 4; ++m) acc[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[m], bh, acc[m][n], 0, 0, 0);
        }

        if (__builtin_expect(ks == nks - 1, 0)) {
            const float* nb = (const float*)(smem + LDS_NORM_OFF + (t & 1) * (TILE_R * 4));
            const int trow0 = (ct0 + t) * TILE_R;
            const int rlim = (int)(p.ntotal - (int64_t)trow0);
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
            // the key, formed here only: n_y + S (IP: S)
            auto key = [&](int m, int n, int i) __attribute__((always_inline)) -> float {
                return METRIC == L2 ? yn[m][i] + acc[m][n][i] : acc[m][n][i];
            };
            int qloc[4];
            bool qv[4];
            float tn[4];
            unsigned pend[4];
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                qloc[n] = tile_qloc(n);
                qv[n] = q0 + qloc[n] < p.nq;
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
                        const float v = key(m, n, i);
                        const int rl = tile_rloc(rl0, m, i);
                        if (qv[n] && rl < rlim && v <= tn[n]) {
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
                                const float v = key(m, n, i);
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

    // final flush: sorted top-KP per query of this (query tile, split)
    __syncthreads();
    const int64_t obase = ((int64_t)qtile * p.splits + split) * TILE_Q;
    for (int q = wave; q < TILE_Q; q += 4) {
        if (q0 + q >= p.nq) break;
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

// ---------------------------------------------------------------------------
// exact arithmetic on decoded rows
// ---------------------------------------------------------------------------
// exact metric value of (x, decoded row) accumulated by `nl` lanes (lane sub of
// nl): lane sub takes dimensions sub, sub + nl, ..
template <int METRIC>
__device__ __forceinline__ double pq_exact_partial(const float* __restrict__ xq, const uint8_t* __restrict__ code,
                                                   int d, int dsub, const float* __restrict__ cb, int sub, int nl) {
    double acc = 0.0;
    for (int j = sub; j < d; j += nl) {
        const int m = j / dsub;
        const double y = (double)cb[((int64_t)m * PQ_KSUB + code[m]) * dsub + (j - m * dsub)];
        if (METRIC == L2) {
            const double df = (double)xq[j] - y;
            acc = fma(df, df, acc);
        } else {
            acc = fma((double)xq[j], y, acc);
        }
    }
    return acc;
}
// the same by one thread, centroid by centroid (no division per dimension)
template <int METRIC>
__device__ __forceinline__ double pq_exact_row(const float* __restrict__ xq, const uint8_t* __restrict__ code, int M,
                                               int dsub, const float* __restrict__ cb) {
    double acc = 0.0;
    for (int m = 0; m < M; ++m) {
        const float* c = cb + ((int64_t)m * PQ_KSUB + code[m]) * dsub;
        const float* xs = xq + m * dsub;
        for (int e = 0; e < dsub; ++e) {
            const double y = (double)c[e];
            if (METRIC == L2) {
                const double df = (double)xs[e] - y;
                acc = fma(df, df, acc);
            } else {
                acc = fma((double)xs[e], y, acc);
            }
        }
    }
    return acc;
}

// merge + exact refine + certification: one wave per query (k_sq_refine's three
// phases over the [qtile][split][TILE_Q][KP] lists; no shared threshold, so
// every split pruned only with its own KP-th key)
template <int METRIC>
__global__ __launch_bounds__(256) void k_pq_refine(PqRefine p) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= p.nq) return;
    const int qtile = (int)(q / TILE_Q), qq = (int)(q % TILE_Q);
    const int ncand = p.splits * KP;

    float bd = FX_INF, td = FX_INF;
    int bi = INT_MAX, ti = INT_MAX;
    int nvalid = 0, bad = 0;
    for (int base = 0; base < ncand; base += 64) {
        const int c = base + lane;
        float d = FX_INF;
        int i = INT_MAX;
        if (c < ncand) {
            const int s = c / KP, j = c - s * KP;
            const int64_t off = (((int64_t)qtile * p.splits + s) * TILE_Q + qq) * KP + j;
            const int ii = p.cand_i[off];
            if (ii >= 0 && ii < p.ntotal) { d = p.cand_d[off]; i = ii; }
            else bad += ii != -1;
        }
        nvalid += __popcll(__ballot(i != INT_MAX));
        const bool pass = i != INT_MAX && key_lt(d, i, td, ti);
        if (!__any(pass)) continue;
        if (!pass) { d = FX_INF; i = INT_MAX; }
        sort64(d, i, lane);
        merge_into(bd, bi, d, i, lane);
        td = __shfl(bd, KP - 1, 64);
        ti = __shfl(bi, KP - 1, 64);
    }
    if (bad != 0 && p.n_drop) atomicAdd(p.n_drop, bad);

    const float* xq = p.qf32 + q * (int64_t)p.kp;
    const int grp = lane >> 4, sub = lane & 15;
    double ex = 0.0;
    for (int r = 0; r < KP / 4; ++r) {
        const int row = __shfl(bi, r * 4 + grp, 64);
        double a = 0.0;
        if (row != INT_MAX)
            a = pq_exact_partial<METRIC>(xq, p.codes + (int64_t)row * p.stride, p.d, p.dsub, p.cb, sub, 16);
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        const double v = __shfl(a, (lane & 3) * 16, 64);
        if ((lane >> 2) == r) ex = v;
    }

    float key = FX_INF;
    int id = INT_MAX;
    if (lane < KP && bi != INT_MAX) {
        key = METRIC == L2 ? (float)ex : -(float)ex;
        id = bi;
    }
    sort64(key, id, lane);
    if (lane < p.k) {
        const bool valid = id != INT_MAX;
        p.D[q * p.k + lane] = valid ? (METRIC == L2 ? key : -key) : (METRIC == L2 ? FLT_MAX : -FLT_MAX);
        p.I[q * p.k + lane] = valid ? (int64_t)id : (int64_t)-1;
    }
    bool flagq = p.force_fb != 0;
    if (!flagq && nvalid >= KP) {  // (fewer than KP candidates in all: no split dropped a row)
        const float kth = __shfl(key, p.k - 1, 64);
        flagq = !sq_certified(kth, td, p.qshift[q], p.qeps[q], 0.0);
    }
    if (flagq && lane == 0) {
        const int pos = atomicAdd(p.n_flag, 1);
        p.n_flag[1 + pos] = (int)q;
    }
}

// ---------------------------------------------------------------------------
// the exact path (k_sq_exact / k_sq_merge over decoded centroids)
// ---------------------------------------------------------------------------
template <int METRIC>
__global__ __launch_bounds__(BT_THREADS) void k_pq_exact(PqExact p) {
    __shared__ float sd[BT_MAXB];
    __shared__ int si[BT_MAXB];
    __shared__ BtState<int> st;
    const int nf = p.n_flag[0];
    if (nf <= 0) return;
    const int* qlist = p.n_flag + 1;
    const int B = bt_cap(p.k);
    const int64_t items = (int64_t)nf * p.xs;
    for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const int f = (int)(w / p.xs), c = (int)(w % p.xs);
        const int64_t q = qlist[f];
        const float* xq = p.qf32 + q * p.kp;
        const int64_t a = p.ntotal * c / p.xs, b = p.ntotal * (c + 1) / p.xs;
        bt_init(&st);
        for (int64_t base = a; base < b; base += BT_THREADS) {
            const int64_t row = base + threadIdx.x;
            const bool valid = row < b;
            float key = FX_INF;
            if (valid) {
                const double v = pq_exact_row<METRIC>(xq, p.codes + row * p.stride, p.M, p.dsub, p.cb);
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
__global__ __launch_bounds__(BT_THREADS) void k_pq_merge(PqExact p) {
    __shared__ float sd[BT_MAXB];
    __shared__ int si[BT_MAXB];
    __shared__ BtState<int> st;
    const int nf = p.n_flag[0];
    if (nf <= 0) return;
    const int* qlist = p.n_flag + 1;
    const int B = bt_cap(p.k);
    const int64_t per = (int64_t)p.xs * p.k;
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
            p.I[q * p.k + t] = valid ? (int64_t)si[t] : (int64_t)-1;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
hipError_t launch_pq_encode(const void* x, int x_dt, int64_t n, int d, int M, int dsub, const float* cb, uint8_t* out,
                            int stride, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (M <= 0 || M > 65535 || dsub <= 0 || M * dsub != d || stride < M) return hipErrorInvalidValue;
    const dim3 grid(pq_grid(n, PQ_THREADS), (unsigned)M);
    if (dsub == 8) hipLaunchKernelGGL(k_pq_encode<8>, grid, dim3(PQ_THREADS), 0, s, x, x_dt, n, d, dsub, cb, out, stride);
    else hipLaunchKernelGGL(k_pq_encode<0>, grid, dim3(PQ_THREADS), 0, s, x, x_dt, n, d, dsub, cb, out, stride);
    return hipGetLastError();
}

hipError_t launch_pq_ny(const uint8_t* codes, int stride, int64_t n, int M, int dsub, const float* cb, float* ny,
                        hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pq_ny, dim3(pq_grid(n, PQ_THREADS)), dim3(PQ_THREADS), 0, s, codes, stride, n, M, dsub, cb, ny);
    return hipGetLastError();
}

hipError_t launch_pq_decode(const uint8_t* codes, int stride, int64_t nrows, const int64_t* keys, int64_t key0,
                            int64_t n, int M, int dsub, const float* cb, float* out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_pq_decode, dim3(pq_grid(n * M * dsub, PQ_THREADS)), dim3(PQ_THREADS), 0, s, codes, stride,
                       nrows, keys, key0, n, M, dsub, cb, out);
    return hipGetLastError();
}

hipError_t launch_pq_prep(const PqPrep& p, hipStream_t s) {
    if (p.nq_pad <= 0 || p.nq_pad % TILE_Q != 0 || p.kp % PQ_STAGE_D != 0 || p.kp < p.d) return hipErrorInvalidValue;
    const double u = 5.9604644775390625e-8;
    // terms accumulated by the scan's fp32 MFMA chain: 3 K products and the key's addition
    const double nt = 3.0 * p.kp + 1.0;
    const double gamma = nt * u / (1.0 - nt * u);
    hipLaunchKernelGGL(k_pq_prep, dim3((unsigned)((p.nq_pad + 3) / 4)), dim3(PQ_THREADS), 0, s, p, gamma);
    return hipGetLastError();
}

hipError_t launch_pq_scan(int metric, const PqScan& p, hipStream_t s) {
    if (p.dsub <= 0 || p.dsub % 8 != 0 || p.M <= 0 || p.M * p.dsub != p.d || p.stride < p.M ||
        p.kp != pq_kpad(p.d) || p.plane_bytes != pq_plane_bytes(p.M, p.dsub) || p.n_qtiles <= 0 || p.splits <= 0 ||
        p.splits > p.n_ctiles || (int64_t)p.n_qtiles * TILE_Q > p.nq_pad ||
        (int64_t)p.n_qtiles * p.splits > (int64_t)INT32_MAX || (int64_t)p.n_ctiles * TILE_R < p.ntotal)
        return hipErrorInvalidValue;
    const int grid = p.n_qtiles * p.splits;
    if (metric == L2) return launch_with_lds(k_pq_scan<L2>, grid, SCAN_THREADS, LDS_SCAN_BYTES, s, p);
    return launch_with_lds(k_pq_scan<IP>, grid, SCAN_THREADS, LDS_SCAN_BYTES, s, p);
}

hipError_t launch_pq_refine(int metric, const PqRefine& p, hipStream_t s) {
    if (p.nq <= 0 || p.k <= 0 || p.k > KP || p.splits <= 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.nq + 3) / 4));
    if (metric == L2) hipLaunchKernelGGL(k_pq_refine<L2>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_pq_refine<IP>, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_pq_exact(int metric, const PqExact& p, hipStream_t s) {
    if (p.k <= 0 || p.k > FX_BIG_K || p.xs <= 0) return hipErrorInvalidValue;
    if (metric == L2) {
        hipLaunchKernelGGL(k_pq_exact<L2>, dim3(PQ_EXACT_GRID), dim3(BT_THREADS), 0, s, p);
        hipLaunchKernelGGL(k_pq_merge<L2>, dim3(PQ_MERGE_GRID), dim3(BT_THREADS), 0, s, p);
    } else {
        hipLaunchKernelGGL(k_pq_exact<IP>, dim3(PQ_EXACT_GRID), dim3(BT_THREADS), 0, s, p);
        hipLaunchKernelGGL(k_pq_merge<IP>, dim3(PQ_MERGE_GRID), dim3(BT_THREADS), 0, s, p);
    }
    return hipGetLastError();
}

}  // namespace fx

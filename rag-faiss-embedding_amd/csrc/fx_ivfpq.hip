// fx_ivfpq.hip -- inverted file over product-quantized codes: faiss's IndexIVFPQ with 8-bit codes
// (by_residual on or off), restated from memory and not checked against a faiss build
// (include/fx_index.h "inverted file over product-quantized codes").
//
// The payload is the inverted file's (rows in LIST ORDER, list l owns rows [list_off[l],
// list_off[l + 1]), fx_ivf.hip) holding the product quantizer's rows (roundup(M, 16) code bytes and
// the row constant n_y = |decode|^2, fx_pq.hip).  With by_residual a code encodes r = fl32(x - c_l),
// c_l the fp32 centroid of the row's list, and the row decodes to y = fl32(c_l + decode(code));
// without it c_l is null everywhere and y = decode(code).  A search ranks the decoded rows of the
// probed lists exactly.  Residuals, the encoder and n_y are the parents' kernels (k_ivfsq_residual,
// k_pq_encode, k_pq_ny); so is the merge of the exact path (k_ivf_merge).
//
//   k_ivfpq_prep   operand preparation, 3.16's split with the list's centroid folded in:
//                L2, by_residual   per (query, probe) pair: x' = -2 fl32(x - c_l) as [hi | lo] bf16
//                                  planes, shift |x - c_l|^2:  |x - y|^2 ~ shift + x'.dec + n_y
//                IP                the operand -x belongs to the query; the pair owns the shift
//                                  -(x . c_l):  -x.y ~ shift + x'.dec
//                no by_residual    IndexPQ's operand and shift, the same for every pair of a query
//                and the pair's bound E.
//   k_ivfpq_scan   k_ivfsq_scan's grid and list logic (one workgroup per (128-pair group of a list,
//                chunk), tile starts aligned down to 4 rows, rows outside the list masked by row
//                number, the flush to cand[q][j * C + chunk][KP]) around k_pq_scan's tile loop (32-
//                dimension stages [A hi | A lo | B hi | B lo], the A side gathered from the codebook
//                image at the address the code byte names, three bf16 MFMAs into one fp32
//                accumulator set, code bytes loaded two stages ahead); the B planes are fetched by
//                the operand row the sorted pair array names.  The epilogue adds the pair's fp32
//                shift to the key, so every candidate key of a query is comparable whatever slot
//                holds it.
//   k_ivfpq_refine   k_ivfsq_refine's three phases; the exact recomputation gathers the candidate's
//                fp32 centroids and adds the centroid of the row's list.
//   k_ivfpq_exact   k_ivf_exact over decoded rows, merged by k_ivf_merge: the flagged queries, every
//                search with KP < k <= FX_BIG_K and every index with dsub % 8 != 0.
#include "fx_sq_common.h"

#include <algorithm>

namespace fx {

namespace {

constexpr int IVFPQ_THREADS = 256;
constexpr int IVFPQ_EXACT_GRID = 1024;
// LDS of k_ivfpq_scan: k_pq_scan's carve, then the group's pair numbers
constexpr int LDS_IVFPQ_PAIR_OFF = LDS_SCAN_BYTES;
constexpr int LDS_IVFPQ_BYTES = LDS_IVFPQ_PAIR_OFF + TILE_Q * 4;
static_assert(LDS_IVFPQ_BYTES <= 160 * 1024, "k_ivfpq_scan's LDS");

}  // namespace

// ---------------------------------------------------------------------------
// operand preparation: one wave per operand row of the padded pass.
//
// The scan key of (pair, row) is  v = fl(a + fl32(shift)),  a = fl(n_y + fl(S))  (IP: fl(S)), S the
// three-product sum of k_pq_prep, and v estimates the exact key of the decoded fp32 row y_f = c_l +
// dec + delta (|delta| <= rho_dec):
//   L2  |v - D| <= E + 2 rho_dec sqrt(D),   E = E_pq(|x'|) + u |x'| Y + u (2 |shift| + Y^2 + A) + rho_dec^2
//   IP  |v + x.y_f| <= E = E_pq(|x'|) + u (2 |shift| + A) + |x| rho_dec
// E_pq is 3.16's bound evaluated with the operand's own |x'|, residual and lo norms; A = 1.03 |x'| Y
// bounds |fl(S)|.  u |x'| Y: the operand holds z = fl32(x - c_l) while the shift is |x - c_l|^2 formed
// in fp64 from the fp32 values (exact), so the key misses 2 (x - c_l - z).dec, at most 2 u |z| Y.  u (2
// |shift| + |a|): the rounding of fl32(shift) and of the one addition, as 3.15's.
// ---------------------------------------------------------------------------
// the [hi | lo] split of operand value xs into the row's planes; rr += |r_x|^2, ll += |x'_lo|^2 of the lane
__device__ __forceinline__ void ivfpq_split(float xs, uint16_t* hi_row, uint16_t* lo_row, int c, double& rr, double& ll) {
    const bool fin = __builtin_isfinite(xs);
    const uint16_t h = f2bf(xs);
    const float hf = bf2f(h);
    const float rest = xs - hf;  // exact in fp32: hi is within 2^-8 |x'| of x'
    const uint16_t l = fin ? f2bf(rest) : (uint16_t)0;
    const double res = (double)rest - (double)bf2f(l);
    hi_row[c] = fin ? h : (uint16_t)0;
    lo_row[c] = l;
    rr += res * res;
    ll += (double)bf2f(l) * (double)bf2f(l);
}

// E of one pair from its operand's norms (xn = |x'|, sqrt(rr), sqrt(ll)), its shift and |x|
__device__ __forceinline__ float ivfpq_eps(const IvfPqPrep& p, double gamma, bool l2, bool folded, double xn, double rr,
                                           double ll, double sh, double xnorm) {
    const double u = 5.9604644775390625e-8;  // 2^-24
    const double A = 1.03 * xn * p.Y;
    double eps = xn * p.Ry + sqrt(rr) * (p.Y + p.Ry) + sqrt(ll) * p.Yl + (gamma + u) * A;
    if (l2) eps += 2.0 * u * p.Y * p.Y;
    eps += u * (2.0 * fabs(sh) + (l2 ? p.Y * p.Y : 0.0) + A) * 1.01;
    if (folded) eps += u * xn * p.Y * 1.01;
    eps += l2 ? p.rho_dec * p.rho_dec : xnorm * p.rho_dec;
    eps += 1e-12 * fabs(sh);
    return (float)(eps * 1.0625 + 1e-30);
}

__global__ __launch_bounds__(IVFPQ_THREADS) void k_ivfpq_prep(IvfPqPrep p, double gamma) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= p.op_rows) return;
    if (r == 0 && lane == 0)
        for (int i = 0; i < 2; ++i)
            if (p.zero[i]) *p.zero[i] = 0;
    const int kp = p.kp, d = p.d;
    const bool l2 = p.metric == L2;
    const float scale = l2 ? -2.0f : -1.0f;
    uint16_t* hi_row = p.planes + r * (int64_t)kp;
    uint16_t* lo_row = p.planes + (p.op_rows + r) * (int64_t)kp;
    const int64_t live_rows = p.per_pair ? p.nq * p.np : p.nq;
    const bool live = r < live_rows;
    const int64_t q = !live ? 0 : p.per_pair ? r / p.np : r;
    const int j0 = (live && p.per_pair) ? (int)(r - q * p.np) : 0;
    // the operand row: fl32(x - c_l) of the pair (per_pair), else x
    const float* cl = nullptr;
    if (live && p.per_pair && p.cent) {
        const int64_t l = p.coarse[r];
        if (l >= 0 && l < p.nlist) cl = p.cent + l * d;
    }
    double xx = 0.0, zz = 0.0, sh = 0.0, rr = 0.0, ll = 0.0;
    for (int c = lane; c < kp; c += 64) {
        const float v = (live && c < d) ? load_elem(p.q, q * d + c, p.q_dt) : 0.0f;
        if (live && j0 == 0) p.qf32[q * (int64_t)kp + c] = v;
        float z = v;
        if (cl && c < d) {
            z = sub_rn(v, cl[c]);
            const double w = (double)v - (double)cl[c];
            sh += w * w;
        }
        const float xs = z == 0.0f ? 0.0f : scale * z;  // (padding and zeros as +0, not -0)
        ivfpq_split(xs, hi_row, lo_row, c, rr, ll);
        xx += (double)v * (double)v;
        zz += (double)z * (double)z;
    }
    xx = wave_sum_f64(xx);
    zz = wave_sum_f64(zz);
    sh = wave_sum_f64(sh);
    rr = wave_sum_f64(rr);
    ll = wave_sum_f64(ll);
    if (!live) return;
    const bool bad = !(xx < 1e300) || !(zz < 1e300);  // (a non-finite query: never certified)
    const double xn = (l2 ? 2.0 : 1.0) * sqrt(zz);    // |x'|
    if (p.per_pair) {
        if (lane != 0) return;
        if (!cl) sh = l2 ? xx : 0.0;
        p.peps[r] = bad ? FX_INF : ivfpq_eps(p, gamma, l2, cl != nullptr, xn, rr, ll, sh, sqrt(xx));
        p.pshift[r] = (float)sh;
        return;
    }
    // the query's operand serves every pair; shift and E are the pair's
    for (int j = 0; j < p.np; ++j) {
        const int64_t pr = q * p.np + j;
        double s = l2 ? xx : 0.0;
        if (p.cent && !l2) {  // IP with by_residual: -(x . c_l)
            const int64_t l = p.coarse[pr];
            double dot = 0.0;
            if (l >= 0 && l < p.nlist)
                for (int c = lane; c < d; c += 64) dot += (double)load_elem(p.q, q * d + c, p.q_dt) * (double)p.cent[l * d + c];
            s = -wave_sum_f64(dot);
        }
        if (lane == 0) {
            p.peps[pr] = bad ? FX_INF : ivfpq_eps(p, gamma, l2, false, xn, rr, ll, s, sqrt(xx));
            p.pshift[pr] = (float)s;
        }
    }
}

// ---------------------------------------------------------------------------
// the list scan.  Per 32-dimension stage the workgroup moves 32 one-KiB pieces: the hi and lo blocks
// of 8 row blocks (A, gathered from the codebook image as k_pq_scan does) and of the group's 8 pair
// blocks (B, the operand rows the pairs name), 4 + 4 per wave.  Every gather address is image + (m *
// 256 + code) * dsub * 2 + piece with m < M and code a byte, so it lies inside the image whatever the
// code bytes hold; the bytes themselves are read at rows below a0 + nt * 128 < list_off[l + 1] + 128,
// inside the allocation's zero tile past the last row.
// ---------------------------------------------------------------------------
template <int METRIC>
__global__ __launch_bounds__(SCAN_THREADS, 1) void k_ivfpq_scan(IvfPqScan p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
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
    const int ct0 = (int)((int64_t)nt * chunk / p.C), ct1 = (int)((int64_t)nt * (chunk + 1) / p.C);
    if (r1 <= r0 || ct0 >= ct1) return;  // (its slots keep the -1 the host wrote)
    const int pos0 = __builtin_amdgcn_readfirstlane(p.seg[l]) + (g - __builtin_amdgcn_readfirstlane(p.gbase[l])) * TILE_Q;
    const int nqg = min(TILE_Q, __builtin_amdgcn_readfirstlane(p.seg[l + 1]) - pos0);  // the group's pairs
    if (nqg <= 0) return;

    float* lst_d = (float*)(smem + LDS_LD_OFF);
    int* lst_i = (int*)(smem + LDS_LI_OFF);
    int* cnt = (int*)(smem + LDS_CNT_OFF);
    float* tau = (float*)(smem + LDS_TAU_OFF);
    volatile int* flag = (volatile int*)(smem + LDS_FLAG_OFF);
    unsigned* pair = (unsigned*)(smem + LDS_IVFPQ_PAIR_OFF);

    for (int x = tid; x < TILE_Q; x += SCAN_THREADS) {
        cnt[x] = 0;
        tau[x] = FX_INF;
        pair[x] = x < nqg ? (unsigned)p.sorted[pos0 + x] : 0xffffffffu;
    }
    if (tid == 0) *flag = 0;
    __syncthreads();

    const int kp = p.kp;
    const int nks = kp / PQ_STAGE_D;
    const int G = (ct1 - ct0) * nks;
    const int s8 = p.dsub >> 3;   // 16-B pieces per centroid
    const int npc = p.d >> 3;     // pieces of a row that hold dimensions
    const int lgrp = lane >> 4;
    const int64_t zoff = p.plane_bytes - 16;  // the zero piece
    const int cmul = p.dsub * 2;              // bytes from one centroid to the next

    // the lane's two A rows of a tile and its two B rows: the operand rows of the pairs that are
    // columns blk * 16 + (lane & 15) of the group; a column past the group reads operand row 0
    int lrow[2];
    int64_t boff[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        lrow[j] = (wave * 2 + j) * 16 + (lane & 15);
        const unsigned pr = pair[lrow[j]];
        const int64_t brow = pr == 0xffffffffu ? 0 : (int64_t)(pr / (unsigned)p.bdiv);
        boff[j] = (brow * kp + lgrp * 8) * 2;
    }
    const char* bplanes = (const char*)p.planes;
    const int64_t bplane = p.op_rows * (int64_t)kp * 2;
    // per pair column: its shift
    float shf[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const unsigned pr = pair[tile_qloc(n)];
        shf[n] = p.pshift[pr == 0xffffffffu ? 0 : (int64_t)pr];
    }

    // what a lane needs to form its two gather addresses of one stage
    struct Gather {
        int64_t base;   // byte offset of centroid 0's piece in a plane (the zero piece: past d)
        int mul;        // cmul, or 0 past d
        unsigned c[2];  // the two rows' code bytes
    };
    auto fetch = [&](int gi) -> Gather {
        const int t = gi / nks, ks = gi - t * nks;
        const int pi = ks * 4 + lgrp;
        const bool has = pi < npc;
        const int m = has ? pi / s8 : 0;
        const int o8 = has ? pi - m * s8 : 0;
        Gather x;
        x.base = has ? ((int64_t)m * PQ_KSUB * p.dsub + o8 * 8) * 2 : zoff;
        x.mul = has ? cmul : 0;
        const uint8_t* cr = p.codes + ((int64_t)a0 + (int64_t)(ct0 + t) * TILE_R) * p.stride + m;
#pragma unroll
        for (int j = 0; j < 2; ++j) x.c[j] = cr[(int64_t)lrow[j] * p.stride];
        return x;
    };
    auto issue = [&](int gi, const Gather& x) {
        const int t = gi / nks, ks = gi - t * nks;
        char* buf = smem + (gi & 1) * PQ_STAGE_BYTES;
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
            glds16(p.ny + (int64_t)a0 + (int64_t)(ct0 + t) * TILE_R + lane * 4, smem + LDS_NORM_OFF + (t & 1) * (TILE_R * 4));
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
    for (int gi = 0; gi < G; ++gi) {
        Gather after{};
        if (gi + 2 < G) after = fetch(gi + 2);
        if (gi + 1 < G) issue(gi + 1, nxt);
        nxt = after;
        const char* buf = smem + (gi & 1) * PQ_STAGE_BYTES;
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
            const int trow0 = a0 + (ct0 + t) * TILE_R;
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
            // the key, formed here only: n_y + S (IP: S), then the pair's shift in one more rounded addition
            auto key = [&](int m, int n, int i) __attribute__((always_inline)) -> float {
                const float a = METRIC == L2 ? add_rn(yn[m][i], acc[m][n][i]) : acc[m][n][i];
                return add_rn(a, shf[n]);
            };
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
                    const int row = trow0 + tile_rloc(rl0, m, i);
                    if (row >= r0 && row < r1) sel |= 1u << (m * 4 + i);
                }
            int ovf = 0;
#pragma unroll
            for (int n = 0; n < 4; ++n)
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float v = key(m, n, i);
                        if (qv[n] && ((sel >> (m * 4 + i)) & 1u) && v <= tn[n]) {
                            const int s = atomicAdd(&cnt[qloc[n]], 1);
                            if (s < CAP) {
                                lst_d[qloc[n] * CAP + s] = v;
                                lst_i[qloc[n] * CAP + s] = trow0 + tile_rloc(rl0, m, i);
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

    // final flush: the sorted top-KP of (this item, pair) -> the query's slot j * C + chunk
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
// exact arithmetic on decoded rows
// ---------------------------------------------------------------------------
// exact metric value of (x, decoded row of a list with centroid cl, or null) accumulated by `nl`
// lanes: lane sub takes dimensions sub, sub + nl, ..; y = fl32(c_l + centroid value)
template <int METRIC>
__device__ __forceinline__ double ivfpq_exact_partial(const float* __restrict__ xq, const uint8_t* __restrict__ code,
                                                      int d, int dsub, const float* __restrict__ cb,
                                                      const float* __restrict__ cl, int sub, int nl) {
    double acc = 0.0;
    for (int j = sub; j < d; j += nl) {
        const int m = j / dsub;
        float yf = cb[((int64_t)m * PQ_KSUB + code[m]) * dsub + (j - m * dsub)];
        if (cl) yf = add_rn(cl[j], yf);
        const double y = (double)yf;
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
__device__ __forceinline__ double ivfpq_exact_row(const float* __restrict__ xq, const uint8_t* __restrict__ code, int d,
                                                  int dsub, const float* __restrict__ cb,
                                                  const float* __restrict__ cl) {
    double acc = 0.0;
    for (int m = 0, j = 0; j < d; ++m) {
        const float* c = cb + ((int64_t)m * PQ_KSUB + code[m]) * dsub;
        for (int e = 0; e < dsub; ++e, ++j) {
            float yf = c[e];
            if (cl) yf = add_rn(cl[j], yf);
            const double y = (double)yf;
            if (METRIC == L2) {
                const double df = (double)xq[j] - y;
                acc = fma(df, df, acc);
            } else {
                acc = fma((double)xq[j], y, acc);
            }
        }
    }
    return acc;
}

// merge + exact refine + certification: one wave per query over its [slots][KP] lists.  Every
// candidate key carries its pair's shift, so keys of different slots compare, and every row a slot
// or the merge dropped has key >= td, the merged KP-th key.
template <int METRIC>
__global__ __launch_bounds__(256) void k_ivfpq_refine(IvfPqRefine p) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= p.nq) return;
    const int ncand = p.slots * KP;

    float bd = FX_INF, td = FX_INF;
    int bi = INT_MAX, ti = INT_MAX;
    int nvalid = 0, bad = 0;
    for (int base = 0; base < ncand; base += 64) {
        const int c = base + lane;
        float d = FX_INF;
        int i = INT_MAX;
        if (c < ncand) {
            const int64_t off = q * ncand + c;
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

    // the query's bound: the largest of its pairs'
    float eq = 0.f;
    for (int j = lane; j < p.np; j += 64) eq = fmaxf(eq, p.peps[q * p.np + j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) eq = fmaxf(eq, __shfl_xor(eq, o, 64));

    const float* xq = p.qf32 + q * (int64_t)p.kp;
    const int grp = lane >> 4, sub = lane & 15;
    double ex = 0.0;
    for (int r = 0; r < KP / 4; ++r) {
        const int row = __shfl(bi, r * 4 + grp, 64);
        double a = 0.0;
        if (row != INT_MAX) {
            const float* cl = nullptr;
            if (p.cent) {
                const int l = p.row_list[row];
                if (l >= 0 && l < p.nlist) cl = p.cent + (int64_t)l * p.d;
            }
            a = ivfpq_exact_partial<METRIC>(xq, p.codes + (int64_t)row * p.stride, p.d, p.dsub, p.cb, cl, sub, 16);
        }
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
        p.I[q * p.k + lane] = valid ? p.labels[id] : (int64_t)-1;
    }
    bool flagq = p.force_fb != 0;
    if (!flagq && nvalid >= KP) {  // (fewer than KP candidates in all: no slot dropped a row)
        const float kth = __shfl(key, p.k - 1, 64);
        flagq = !sq_certified(kth, td, 0.0, eq, METRIC == L2 ? p.rho_dec : 0.0);
    }
    if (flagq && lane == 0) {
        const int pos = atomicAdd(p.n_flag, 1);
        p.n_flag[1 + pos] = (int)q;
    }
}

// ---------------------------------------------------------------------------
// the exact path: k_ivf_exact over decoded rows (fx_ivf.hip); k_ivf_merge ranks its lists
// ---------------------------------------------------------------------------
template <int METRIC>
__global__ __launch_bounds__(BT_THREADS) void k_ivfpq_exact(IvfPqExact pp) {
    __shared__ float sd[BT_MAXB];
    __shared__ int si[BT_MAXB];
    __shared__ BtState<int> st;
    const IvfExact& p = pp.ex;
    const int nf = p.n_flag[0];
    if (nf <= 0) return;
    const int* qlist = p.n_flag + 1;
    const int slots = p.np * p.C, B = bt_cap(p.k);
    const int64_t items = (int64_t)nf * slots;
    const uint8_t* codes = (const uint8_t*)p.codes;
    for (int64_t w = blockIdx.x; w < items; w += gridDim.x) {
        const int f = (int)(w / slots), slot = (int)(w % slots);
        const int j = slot / p.C, c = slot % p.C;
        const int64_t q = qlist[f];
        const float* xq = p.qf32 + q * p.kdim;
        const int64_t l = p.coarse[q * p.np + j];
        int64_t a = 0, b = 0;  // the chunk's rows (none for a list number outside the index)
        const float* cl = nullptr;
        if (l >= 0 && l < p.nlist) {
            const int64_t r0 = p.list_off[l], r1 = p.list_off[l + 1];
            a = r0 + (r1 - r0) * c / p.C;
            b = r0 + (r1 - r0) * (c + 1) / p.C;
            if (pp.cent) cl = pp.cent + l * pp.d;
        }
        bt_init(&st);
        for (int64_t base = a; base < b; base += BT_THREADS) {
            const int64_t row = base + threadIdx.x;
            const bool valid = row < b;
            float key = FX_INF;
            if (valid) {
                const double v = ivfpq_exact_row<METRIC>(xq, codes + row * p.row_bytes, pp.d, pp.dsub, pp.cb, cl);
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

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
hipError_t launch_ivfpq_prep(const IvfPqPrep& p, hipStream_t s) {
    if (p.nq <= 0 || p.np <= 0 || p.kp % PQ_STAGE_D != 0 || p.kp < p.d ||
        p.op_rows < (p.per_pair ? p.nq * p.np : p.nq))
        return hipErrorInvalidValue;
    const double u = 5.9604644775390625e-8;
    // terms accumulated by the scan's fp32 MFMA chain: 3 K products and the key's addition
    const double nt = 3.0 * p.kp + 1.0;
    const double gamma = nt * u / (1.0 - nt * u);
    hipLaunchKernelGGL(k_ivfpq_prep, dim3((unsigned)((p.op_rows + 3) / 4)), dim3(IVFPQ_THREADS), 0, s, p, gamma);
    return hipGetLastError();
}

hipError_t launch_ivfpq_scan(int metric, const IvfPqScan& p, hipStream_t s) {
    if (p.dsub <= 0 || p.dsub % 8 != 0 || p.M <= 0 || p.M * p.dsub != p.d || p.stride < p.M || p.kp != pq_kpad(p.d) ||
        p.plane_bytes != pq_plane_bytes(p.M, p.dsub) || p.grid <= 0 || p.grid > (int64_t)INT32_MAX || p.np <= 0 ||
        p.C <= 0 || p.nlist <= 0 || p.op_rows <= 0 || (p.bdiv != 1 && p.bdiv != p.np))
        return hipErrorInvalidValue;
    if (metric == L2) return launch_with_lds(k_ivfpq_scan<L2>, (int)p.grid, SCAN_THREADS, LDS_IVFPQ_BYTES, s, p);
    return launch_with_lds(k_ivfpq_scan<IP>, (int)p.grid, SCAN_THREADS, LDS_IVFPQ_BYTES, s, p);
}

hipError_t launch_ivfpq_refine(int metric, const IvfPqRefine& p, hipStream_t s) {
    if (p.nq <= 0 || p.k <= 0 || p.k > KP || p.slots <= 0 || p.np <= 0 || !p.labels || !p.row_list)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.nq + 3) / 4));
    if (metric == L2) hipLaunchKernelGGL(k_ivfpq_refine<L2>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_ivfpq_refine<IP>, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_ivfpq_exact(int metric, const IvfPqExact& p, hipStream_t s) {
    if (p.ex.k <= 0 || p.ex.k > FX_BIG_K || p.ex.np <= 0 || p.ex.C <= 0 || !p.ex.labels || p.dsub <= 0)
        return hipErrorInvalidValue;
    if (metric == L2) hipLaunchKernelGGL(k_ivfpq_exact<L2>, dim3(IVFPQ_EXACT_GRID), dim3(BT_THREADS), 0, s, p);
    else hipLaunchKernelGGL(k_ivfpq_exact<IP>, dim3(IVFPQ_EXACT_GRID), dim3(BT_THREADS), 0, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_ivf_merge(metric, p.ex, s);
}

}  // namespace fx

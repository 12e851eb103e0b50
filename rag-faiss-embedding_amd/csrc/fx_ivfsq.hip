// fx_ivfsq.hip -- inverted file over 8-bit codes: faiss's IndexIVFScalarQuantizer (QT_8bit,
// QT_8bit_uniform; by_residual on or off), restated from memory and not checked against a faiss
// build (include/fx_index.h "inverted file over 8-bit codes").
//
// The payload is the inverted file's (rows in LIST ORDER, list l owns rows [list_off[l],
// list_off[l + 1]), fx_ivf.hip) holding the scalar quantizer's rows (signed codes c' = c - 128 in
// rows of roundup(d, 128) bytes and the row constant n_c, fx_sq.hip).  With by_residual a code
// encodes r = fl32(x - c_l), c_l the fp32 centroid of the row's list, and the row decodes to y =
// fl32(c_l + decode(code)); without it c_l is null everywhere and y = decode(code).  A search ranks
// the decoded rows of the probed lists exactly.
//
//   k_ivfsq_residual   (x, list, centroids) -> fl32(x - c): feeds training (k_sq_minmax) and
//                encoding (k_sq_encode), chunk by chunk.
//   k_ivfsq_consts   rho_dec of a decoded row: k_sq_consts' term plus the rounding of the
//                centroid's addition.
//   k_ivfsq_prep   operand preparation per (query, probe) pair: 3.14's algebra with the list's
//                centroid folded in,
//                L2  z = x - c_l - m, w = z o s, |x - y|^2 = |z|^2 - 2 w.c' + n_c
//                IP  w = x o s,                  x.y       = x.(c_l + m) + w.c'
//                so planes, sigma, shift and E belong to the pair q * np + j.
//   k_ivfsq_scan   k_ivf_scan's grid and list logic (one workgroup per (128-pair group of a list,
//                chunk), tile starts aligned down to 4 rows, rows outside the list masked by row
//                number, the flush to cand[q][j * C + chunk][KP]) around k_sq_scan's tile loop
//                (64-B stages, three i32 accumulator sets on v_mfma_i32_16x16x64_i8, the key formed
//                in the epilogue only); the B planes are fetched by the pair number the sorted pair
//                array names.  The epilogue adds the pair's fp32 shift to the key, so every
//                candidate key of a query is comparable whatever slot holds it.
//   k_ivfsq_refine   k_sq_refine's three phases over [nq][slots][KP] with shift 0 and E = the
//                largest of the query's pairs'; the exact recomputation decodes the candidate's
//                bytes and adds the centroid of the row's list.
//   k_ivfsq_exact   k_ivf_exact over decoded rows, merged by k_ivf_merge: the flagged queries and
//                every search with KP < k <= FX_BIG_K.
#include "fx_sq_common.h"

#include <algorithm>

namespace fx {

namespace {

constexpr int IVFSQ_THREADS = 256;
constexpr int IVFSQ_GRID_CAP = 4096;
constexpr int IVFSQ_EXACT_GRID = 1024;
// LDS of k_ivfsq_scan: k_sq_scan's carve, then the group's pair numbers
constexpr int LDS_IVFSQ_PAIR_OFF = LDS_SCAN_BYTES;
constexpr int LDS_IVFSQ_BYTES = LDS_IVFSQ_PAIR_OFF + TILE_Q * 4;
static_assert(LDS_IVFSQ_BYTES <= 160 * 1024, "k_ivfsq_scan's LDS");

unsigned ivfsq_grid(int64_t items, int per_block) {
    const int64_t g = (items + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : g > IVFSQ_GRID_CAP ? IVFSQ_GRID_CAP : g);
}

}  // namespace

// ---------------------------------------------------------------------------
// residuals, constants, list codes
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(IVFSQ_THREADS) void k_ivfsq_residual(const void* __restrict__ x, int x_dt, int64_t n,
                                                                  int d, const int* __restrict__ row_list,
                                                                  int64_t nlist, const float* __restrict__ cent,
                                                                  float* __restrict__ out) {
    const int64_t items = n * d;
    for (int64_t e = (int64_t)blockIdx.x * IVFSQ_THREADS + threadIdx.x; e < items;
         e += (int64_t)gridDim.x * IVFSQ_THREADS) {
        const int64_t i = e / d;
        const int j = (int)(e - i * d);
        const int l = row_list[i];
        const float v = load_elem(x, e, x_dt);
        out[e] = (l >= 0 && l < nlist) ? sub_rn(v, cent[(int64_t)l * d + j]) : v;
    }
}

// k_sq_consts with the centroid's addition: y = fl32(c_l + dec), |y - (c_l + dec)| <= u |c_l + dec|
// <= u (max_l |c_lj| + max |dec_j|) per dimension
__global__ __launch_bounds__(IVFSQ_THREADS) void k_ivfsq_consts(const float* __restrict__ trained, int d,
                                                                const float* __restrict__ cent, int64_t nlist,
                                                                unsigned* __restrict__ words) {
    __shared__ double part[IVFSQ_THREADS / 64];
    double a = 0.0;
    for (int c = threadIdx.x; c < d; c += IVFSQ_THREADS) {
        const double vmin = trained[c], vdiff = trained[d + c];
        const double ymax = fmax(fabs(vmin), fabs(vmin + vdiff));
        double cmax = 0.0;
        for (int64_t l = 0; l < nlist; ++l) cmax = fmax(cmax, fabs((double)cent[l * d + c]));
        const double u = 5.9604644775390625e-8;
        const double dj = u * (2.0 * vdiff + ymax) * 1.001 + 1e-44 + u * (cmax + ymax * 1.000001) * 1.001;
        a += dj * dj;
    }
    a = wave_sum_f64(a);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < IVFSQ_THREADS / 64; ++w) t += part[w];
        words[SQ_W_RHO] = __float_as_uint((float)(sqrt(t) * 1.000001));
    }
}

__global__ __launch_bounds__(IVFSQ_THREADS) void k_ivfsq_codes_u8(const char* __restrict__ codes, int row_bytes,
                                                                  int64_t r0, int64_t n, int d,
                                                                  uint8_t* __restrict__ out) {
    const int64_t items = n * d;
    for (int64_t e = (int64_t)blockIdx.x * IVFSQ_THREADS + threadIdx.x; e < items;
         e += (int64_t)gridDim.x * IVFSQ_THREADS) {
        const int64_t i = e / d;
        const int j = (int)(e - i * d);
        out[e] = (uint8_t)((unsigned char)codes[(r0 + i) * row_bytes + j] ^ 0x80u);
    }
}

// ---------------------------------------------------------------------------
// operand preparation: one wave per pair row of the padded pass.
//
// The scan key of (pair, row) is  v = fl(a + fl32(shift)),  a = fl(n_c) - 2 sigma fl(S)  (IP:
// -sigma fl(S)) as k_sq_prep describes, and v estimates the exact key of the decoded fp32 row y_f =
// c_l + m + s o c' + delta (|delta| <= rho_dec, k_ivfsq_consts):
//   L2  |v - D| <= E + 2 rho_dec sqrt(D),   E = 2 rho' C + u (2 M^2 + 8 A) + rho_dec^2 + u (2 |shift| + M^2 + 2 A)
//   IP  |v + x.y_f| <= E = rho' C + 3 u A + |x| rho_dec + u (2 |shift| + A)
// The last term is new: fl32(shift) costs u |shift|, and the addition u |a + fl32(shift)| <= u (|a|
// + |shift|) with |a| <= M^2 + 2 A (IP: A).  z is formed in fp64 from the fp32 x, c_l and the
// table, so the pair's operand sees the centroid exactly.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(IVFSQ_THREADS) void k_ivfsq_prep(IvfSqPrep p) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= p.pairs_pad) return;
    if (r == 0 && lane == 0)
        for (int i = 0; i < 2; ++i)
            if (p.zero[i]) *p.zero[i] = 0;
    const int64_t npairs = p.nq * p.np;
    const bool live = r < npairs;
    const int64_t q = live ? r / p.np : 0;
    const int j = live ? (int)(r - q * p.np) : 0;
    const int rb = p.row_bytes, d = p.d;
    const bool l2 = p.metric == L2;
    const float* cl = nullptr;
    if (live && p.cent) {
        const int64_t l = p.coarse[r];
        if (l >= 0 && l < p.nlist) cl = p.cent + l * d;
    }
    double sh = 0.0, xx = 0.0, wmax = 0.0;
    for (int c = lane; c < rb; c += 64) {
        const float v = (live && c < d) ? load_elem(p.q, q * d + c, p.q_dt) : 0.0f;
        if (live && j == 0) p.qf32[q * (int64_t)rb + c] = v;
        if (c < d) {
            double m, s;
            sq_affine(p.trained, d, c, m, s);
            if (cl) m += (double)cl[c];
            const double zv = l2 ? (double)v - m : (double)v;
            wmax = fmax(wmax, fabs(zv * s));
            sh += l2 ? zv * zv : (double)v * m;
            xx += (double)v * (double)v;
        }
    }
    wmax = wave_max_f64(wmax);
    sh = wave_sum_f64(sh);
    xx = wave_sum_f64(xx);
    const bool bad = !(wmax < 1e300) || !(xx < 1e300);  // (a non-finite query: never certified)
    double sg = 1.0;
    if (live && !bad && wmax > 0.0) {
        int e;
        const double f = frexp(wmax / 127.0, &e);  // f in [0.5, 1)
        int ce = f == 0.5 ? e - 1 : e;             // ceil(log2(wmax / 127))
        ce = ce < -120 ? -120 : ce > 120 ? 120 : ce;
        sg = ldexp(1.0, ce);
    }
    double h1s = 0.0, h2s = 0.0, h3s = 0.0, res2 = 0.0;
    for (int c = lane; c < rb; c += 64) {
        double w = 0.0;
        if (live && !bad && c < d) {
            double m, s;
            sq_affine(p.trained, d, c, m, s);
            if (cl) m += (double)cl[c];
            const float v = load_elem(p.q, q * d + c, p.q_dt);
            w = (l2 ? (double)v - m : (double)v) * s;
        }
        const double r1 = w / sg, h1 = sq_digit(r1);
        const double r2 = (r1 - h1) * 256.0, h2 = sq_digit(r2);
        const double r3 = (r2 - h2) * 256.0, h3 = sq_digit(r3);
        const double rs = (r3 - h3) * (sg / 65536.0);
        h1s += h1 * h1;
        h2s += h2 * h2;
        h3s += h3 * h3;
        res2 += rs * rs;
        p.planes[((int64_t)0 * p.pairs_pad + r) * rb + c] = (char)(int)h1;
        p.planes[((int64_t)1 * p.pairs_pad + r) * rb + c] = (char)(int)h2;
        p.planes[((int64_t)2 * p.pairs_pad + r) * rb + c] = (char)(int)h3;
    }
    h1s = wave_sum_f64(h1s);
    h2s = wave_sum_f64(h2s);
    h3s = wave_sum_f64(h3s);
    res2 = wave_sum_f64(res2);
    if (lane != 0) return;
    p.sigma[r] = (float)sg;
    const double u = 5.9604644775390625e-8;  // 2^-24
    const double C = sqrt((double)p.words[SQ_W_MAXC2]);
    const double M2 = (double)__uint_as_float(p.words[SQ_W_MAXNC]);
    const double rdec = (double)__uint_as_float(p.words[SQ_W_RHO]);
    const double A = sg * (sqrt(h1s) + sqrt(h2s) / 256.0 + sqrt(h3s) / 65536.0) * C;
    const double rp = sqrt(res2);
    double eps;
    if (l2)
        eps = 2.0 * rp * C + u * (2.0 * M2 + 8.0 * A) * 1.01 + rdec * rdec + 1e-12 * sh +
              u * (2.0 * sh + M2 + 2.0 * A) * 1.01;
    else
        eps = rp * C + 3.0 * u * A * 1.01 + sqrt(xx) * rdec + 1e-12 * fabs(sh) + u * (2.0 * fabs(sh) + A) * 1.01;
    p.peps[r] = !live ? 0.f : bad ? FX_INF : (float)(eps * 1.0625 + 1e-30);
    p.pshift[r] = !live ? 0.f : (float)(l2 ? sh : -sh);
}

// ---------------------------------------------------------------------------
// the list scan.  Per 64-B stage the workgroup moves 8 one-KiB pieces of code rows and 24 pieces
// of the group's three planes (k_sq_scan's layout); the lane's six B rows are those of the pairs
// that are columns qblk * 16 + (lane & 15) of the group.
// ---------------------------------------------------------------------------
template <int METRIC>
__global__ __launch_bounds__(SCAN_THREADS, 1) void k_ivfsq_scan(IvfSqScan p) {
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
    unsigned* pair = (unsigned*)(smem + LDS_IVFSQ_PAIR_OFF);

    for (int x = tid; x < TILE_Q; x += SCAN_THREADS) {
        cnt[x] = 0;
        tau[x] = FX_INF;
        pair[x] = x < nqg ? (unsigned)p.sorted[pos0 + x] : 0xffffffffu;
    }
    if (tid == 0) *flag = 0;
    __syncthreads();

    const int rb = p.row_bytes;
    const int nks = rb / SQ_STAGE_B;
    const int G = (ct1 - ct0) * nks;

    int aoff[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) aoff[j] = ((wave * 2 + j) * 16 + (lane & 15)) * rb + (lane >> 4) * 16;
    // the lane's six B rows; a column past the group reads pair 0 of the pass (never pushed)
    int64_t boff[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int bi = wave * 6 + j, plane = bi >> 3, qblk = bi & 7;
        const unsigned pr = pair[qblk * 16 + (lane & 15)];
        const int64_t prow = pr == 0xffffffffu ? 0 : (int64_t)pr;
        boff[j] = ((int64_t)plane * p.pairs_pad + prow) * rb + (lane >> 4) * 16;
    }
    // per pair column: the key's scale -2 sigma (L2), -sigma (IP), a power of two; and its shift
    float sg[4], shf[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
        const unsigned pr = pair[tile_qloc(n)];
        const int64_t prow = pr == 0xffffffffu ? 0 : (int64_t)pr;
        sg[n] = (METRIC == L2 ? -2.0f : -1.0f) * p.sigma[prow];
        shf[n] = p.pshift[prow];
    }

    auto issue = [&](int gi) {
        const int t = gi / nks, ks = gi - t * nks;
        char* buf = smem + (gi & 1) * SQ_STAGE_BYTES;
        const int64_t row0 = (int64_t)a0 + (int64_t)(ct0 + t) * TILE_R;
        const char* abase = p.codes + row0 * rb + ks * SQ_STAGE_B;
        const char* bbase = p.planes + ks * SQ_STAGE_B;
#pragma unroll
        for (int j = 0; j < 2; ++j) glds16(abase + aoff[j], buf + (wave * 2 + j) * 1024);
#pragma unroll
        for (int j = 0; j < 6; ++j) glds16(bbase + boff[j], buf + TILE_R * SQ_STAGE_B + (wave * 6 + j) * 1024);
        if (METRIC == L2 && ks == 0 && wave == 0 && lane < 32)
            glds16(p.nc + row0 + lane * 4, smem + LDS_NORM_OFF + (t & 1) * (TILE_R * 4));
    };

    i32x4 acc[SQ_P][4][4];
#pragma unroll
    for (int pl = 0; pl < SQ_P; ++pl)
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int n = 0; n < 4; ++n) acc[pl][m][n] = i32x4{0, 0, 0, 0};

    if (G > 0) issue(0);
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");

    int t = 0, ks = 0;
    for (int gi = 0; gi < G; ++gi) {
        if (gi + 1 < G) issue(gi + 1);
        const char* buf = smem + (gi & 1) * SQ_STAGE_BYTES;
        i32x4 a[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) a[m] = *(const i32x4*)(buf + (wm * 4 + m) * 1024 + lane * 16);
#pragma unroll
        for (int pl = 0; pl < SQ_P; ++pl)
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const i32x4 b = *(const i32x4*)(buf + TILE_R * SQ_STAGE_B + (pl * 8 + wn * 4 + n) * 1024 + lane * 16);
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    acc[pl][m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[m], b, acc[pl][m][n], 0, 0, 0);
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
            // the key, formed here only: fl(n_c - 2 sigma (f32(a1) + f32(a2) / 256 + f32(a3) / 65536)), then
            // the pair's shift in one more rounded addition
            auto key = [&](int m, int n, int i) __attribute__((always_inline)) -> float {
                const float s = fmaf((float)acc[2][m][n][i], 1.0f / 65536.0f,
                                     fmaf((float)acc[1][m][n][i], 1.0f / 256.0f, (float)acc[0][m][n][i]));
                const float a = METRIC == L2 ? fmaf(sg[n], s, yn[m][i]) : sg[n] * s;
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
            for (int pl = 0; pl < SQ_P; ++pl)
#pragma unroll
                for (int m = 0; m < 4; ++m)
#pragma unroll
                    for (int n = 0; n < 4; ++n) acc[pl][m][n] = i32x4{0, 0, 0, 0};
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
// lanes (lane sub of nl), 16 codes per step
template <int METRIC>
__device__ __forceinline__ double ivfsq_exact_partial(const float* __restrict__ xq, const char* __restrict__ row, int d,
                                                      const float* __restrict__ trained,
                                                      const float* __restrict__ cl, int sub, int nl) {
    double acc = 0.0;
    for (int c = sub; c * 16 < d; c += nl) {
        const uint4 raw = *(const uint4*)(row + c * 16);
        const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int j = c * 16 + e;
            if (j < d) {
                const int cs = (int)(signed char)((w[e >> 2] >> (8 * (e & 3))) & 0xffu);
                float yf = sq_decode1(cs, trained[j], trained[d + j]);
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
    }
    return acc;
}

// merge + exact refine + certification: one wave per query over its [slots][KP] lists.  Every
// candidate key carries its pair's shift, so keys of different slots compare, and every row a slot
// or the merge dropped has key >= td, the merged KP-th key.
template <int METRIC>
__global__ __launch_bounds__(256) void k_ivfsq_refine(IvfSqRefine p) {
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

    const float* xq = p.qf32 + q * (int64_t)p.row_bytes;
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
            a = ivfsq_exact_partial<METRIC>(xq, p.codes + (int64_t)row * p.row_bytes, p.d, p.trained, cl, sub, 16);
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
        const double rho = METRIC == L2 ? (double)__uint_as_float(p.words[SQ_W_RHO]) : 0.0;
        flagq = !sq_certified(kth, td, 0.0, eq, rho);
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
__global__ __launch_bounds__(BT_THREADS) void k_ivfsq_exact(IvfSqExact pp) {
    __shared__ float sd[BT_MAXB];
    __shared__ int si[BT_MAXB];
    __shared__ BtState<int> st;
    const IvfExact& p = pp.ex;
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
                const double v =
                    ivfsq_exact_partial<METRIC>(xq, p.codes + row * p.row_bytes, pp.d, pp.trained, cl, 0, 1);
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
hipError_t launch_ivfsq_residual(const void* x, int x_dt, int64_t n, int d, const int* row_list, int64_t nlist,
                                 const float* cent, float* out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (!cent || !row_list) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ivfsq_residual, dim3(ivfsq_grid(n * d, IVFSQ_THREADS)), dim3(IVFSQ_THREADS), 0, s, x, x_dt, n,
                       d, row_list, nlist, cent, out);
    return hipGetLastError();
}

hipError_t launch_ivfsq_consts(const float* trained, int d, const float* cent, int64_t nlist, unsigned* words,
                               hipStream_t s) {
    if (!cent) return launch_sq_consts(trained, d, words, s);
    hipLaunchKernelGGL(k_ivfsq_consts, dim3(1), dim3(IVFSQ_THREADS), 0, s, trained, d, cent, nlist, words);
    return hipGetLastError();
}

hipError_t launch_ivfsq_codes_u8(const char* codes, int row_bytes, int64_t r0, int64_t n, int d, uint8_t* out,
                                 hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ivfsq_codes_u8, dim3(ivfsq_grid(n * d, IVFSQ_THREADS)), dim3(IVFSQ_THREADS), 0, s, codes,
                       row_bytes, r0, n, d, out);
    return hipGetLastError();
}

hipError_t launch_ivfsq_prep(const IvfSqPrep& p, hipStream_t s) {
    if (p.nq <= 0 || p.np <= 0 || p.pairs_pad < p.nq * p.np || p.row_bytes % ROW_ALIGN != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ivfsq_prep, dim3((unsigned)((p.pairs_pad + 3) / 4)), dim3(IVFSQ_THREADS), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_ivfsq_scan(int metric, const IvfSqScan& p, hipStream_t s) {
    if (p.row_bytes <= 0 || p.row_bytes % ROW_ALIGN != 0 || p.grid <= 0 || p.grid > (int64_t)INT32_MAX || p.np <= 0 ||
        p.C <= 0 || p.nlist <= 0 || p.pairs_pad <= 0)
        return hipErrorInvalidValue;
    if (metric == L2) return launch_with_lds(k_ivfsq_scan<L2>, (int)p.grid, SCAN_THREADS, LDS_IVFSQ_BYTES, s, p);
    return launch_with_lds(k_ivfsq_scan<IP>, (int)p.grid, SCAN_THREADS, LDS_IVFSQ_BYTES, s, p);
}

hipError_t launch_ivfsq_refine(int metric, const IvfSqRefine& p, hipStream_t s) {
    if (p.nq <= 0 || p.k <= 0 || p.k > KP || p.slots <= 0 || p.np <= 0 || !p.labels || !p.row_list)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.nq + 3) / 4));
    if (metric == L2) hipLaunchKernelGGL(k_ivfsq_refine<L2>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_ivfsq_refine<IP>, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_ivfsq_exact(int metric, const IvfSqExact& p, hipStream_t s) {
    if (p.ex.k <= 0 || p.ex.k > FX_BIG_K || p.ex.np <= 0 || p.ex.C <= 0 || !p.ex.labels) return hipErrorInvalidValue;
    if (metric == L2) hipLaunchKernelGGL(k_ivfsq_exact<L2>, dim3(IVFSQ_EXACT_GRID), dim3(BT_THREADS), 0, s, p);
    else hipLaunchKernelGGL(k_ivfsq_exact<IP>, dim3(IVFSQ_EXACT_GRID), dim3(BT_THREADS), 0, s, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_ivf_merge(metric, p.ex, s);
}

}  // namespace fx

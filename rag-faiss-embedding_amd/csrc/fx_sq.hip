// fx_sq.hip -- scalar quantizer: faiss's IndexScalarQuantizer with 8-bit codes
// (QT_8bit, QT_8bit_uniform), restated from memory and not checked against a
// faiss build (include/fx_index.h "scalar quantizer").
//
// A row is one byte per dimension, c = trunc(255 clamp((x - vmin) / vdiff, 0,
// 1)), stored as the signed code c' = c - 128 (faiss's byte XOR 0x80) in rows of
// roundup(d, 128) bytes; it decodes to y = vmin + ((c + 0.5) / 255) vdiff (two
// rounded fp32 operations on the table value).  A search ranks the DECODED rows
// exactly, as the flat index ranks its stored rows.
//
//   k_sq_minmax / k_sq_finish   training: per-dimension min / max by order-
//                preserving integer atomics (order-independent, so bitwise
//                reproducible), non-finite inputs counted in the same pass.
//   k_sq_encode  add: the signed codes, the row constant n_c = sum (s_j c'_j)^2
//                (s = vdiff / 255; fp64 sum rounded once) and the running
//                maxima of n_c and of sum c'^2.
//   k_sq_prep    with y = m + s o c' (m = vmin + 128.5 s, the box centre):
//                L2  z = x - m, w = z o s, |x - y|^2 = |z|^2 - 2 w.c' + n_c
//                IP  w = x o s,            x.y       = x.m + w.c'
//                the operand w as SQ_P = 3 int8 digit planes with a per-query
//                power-of-two scale sigma, and the query's bound E.
//   k_sq_scan    a sibling of scan_tiles_128 + k_scan_topk: 128 code rows x 128
//                queries per tile, 64-B stages (one k-chunk of the int8 MFMA),
//                v_mfma_i32_16x16x64_i8 into one i32 accumulator set per plane;
//                the key is formed in the epilogue only.
//   k_sq_refine  k_refine's merge, exact recomputation (decoding the candidate's
//                bytes) and certification, without a shared threshold.
//   k_sq_exact / k_sq_merge   the exact path: fp64 distances of every decoded
//                row, block top-k, per-query merge under (key, row).  Serves the
//                flagged queries and every search with KP < k <= FX_BIG_K:
//                correct, but one fp64 pass over every row.
//   k_sq_encode_u8 / k_sq_decode   the codec (sa_encode, sa_decode, reconstruct).
#include "fx_sq_common.h"

#include <algorithm>

namespace fx {

namespace {

constexpr int SQ_THREADS = 256;
constexpr int SQ_GRID_CAP = 4096;

unsigned sq_grid(int64_t items, int per_block) {
    const int64_t g = (items + per_block - 1) / per_block;
    return (unsigned)(g < 1 ? 1 : g > SQ_GRID_CAP ? SQ_GRID_CAP : g);
}

}  // namespace

// ---------------------------------------------------------------------------
// training
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(SQ_THREADS) void k_sq_minmax_reset(unsigned* __restrict__ mm, int d,
                                                                unsigned long long* __restrict__ bad) {
    for (int c = blockIdx.x * SQ_THREADS + threadIdx.x; c < 2 * d; c += gridDim.x * SQ_THREADS)
        mm[c] = c < d ? 0xffffffffu : 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) *bad = 0ull;
}

// a workgroup takes a run of rows, a thread the columns t, t + 256, ..
__global__ __launch_bounds__(SQ_THREADS) void k_sq_minmax(const void* __restrict__ x, int x_dt, int64_t n, int d,
                                                          unsigned* __restrict__ mm,
                                                          unsigned long long* __restrict__ bad) {
    const int64_t per = (n + gridDim.x - 1) / gridDim.x;
    const int64_t r0 = (int64_t)blockIdx.x * per, r1 = min(n, r0 + per);
    unsigned long long nb = 0ull;
    for (int c = threadIdx.x; c < d; c += SQ_THREADS) {
        unsigned lo = 0xffffffffu, hi = 0u;
        for (int64_t r = r0; r < r1; ++r) {
            const float v = load_elem(x, r * d + c, x_dt);
            if (!__builtin_isfinite(v)) { ++nb; continue; }
            const unsigned o = f2ord(v);
            lo = o < lo ? o : lo;
            hi = o > hi ? o : hi;
        }
        if (lo <= hi) {
            atomicMin(mm + c, lo);
            atomicMax(mm + d + c, hi);
        }
    }
    if (nb) atomicAdd(bad, nb);
}

__global__ __launch_bounds__(SQ_THREADS) void k_sq_finish(const unsigned* __restrict__ mm, int d, int uniform,
                                                          float* __restrict__ trained) {
    __shared__ unsigned slo[SQ_THREADS], shi[SQ_THREADS];
    unsigned lo = 0xffffffffu, hi = 0u;
    if (uniform) {
        for (int c = threadIdx.x; c < d; c += SQ_THREADS) {
            lo = min(lo, mm[c]);
            hi = max(hi, mm[d + c]);
        }
        slo[threadIdx.x] = lo;
        shi[threadIdx.x] = hi;
        __syncthreads();
        for (int o = SQ_THREADS / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) {
                slo[threadIdx.x] = min(slo[threadIdx.x], slo[threadIdx.x + o]);
                shi[threadIdx.x] = max(shi[threadIdx.x], shi[threadIdx.x + o]);
            }
            __syncthreads();
        }
        lo = slo[0];
        hi = shi[0];
    }
    for (int c = threadIdx.x; c < d; c += SQ_THREADS) {
        const unsigned l = uniform ? lo : mm[c], h = uniform ? hi : mm[d + c];
        const float vmin = l <= h ? ord2f(l) : 0.f;  // (a dimension no finite value reached)
        trained[c] = vmin;
        trained[d + c] = l <= h ? ord2f(h) - vmin : 0.f;
    }
}

// rho_dec: the decoded fp32 row differs from m + s c' by the decode's three
// roundings, per dimension <= u (2 vdiff + max |y|) (1 + small)
__global__ __launch_bounds__(SQ_THREADS) void k_sq_consts(const float* __restrict__ trained, int d,
                                                          unsigned* __restrict__ words) {
    __shared__ double part[SQ_THREADS / 64];
    double a = 0.0;
    for (int c = threadIdx.x; c < d; c += SQ_THREADS) {
        const double vmin = trained[c], vdiff = trained[d + c];
        const double dj = 5.9604644775390625e-8 * (2.0 * vdiff + fmax(fabs(vmin), fabs(vmin + vdiff))) * 1.001 + 1e-44;
        a += dj * dj;
    }
    a = wave_sum_f64(a);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        for (int w = 0; w < SQ_THREADS / 64; ++w) t += part[w];
        words[SQ_W_RHO] = __float_as_uint((float)(sqrt(t) * 1.000001));
    }
}

// ---------------------------------------------------------------------------
// encode / decode
// ---------------------------------------------------------------------------
// one wave per row
__global__ __launch_bounds__(SQ_THREADS) void k_sq_encode(const void* __restrict__ x, int x_dt, int64_t n, int d,
                                                          const float* __restrict__ trained, int row_bytes,
                                                          char* __restrict__ codes, float* __restrict__ nc,
                                                          unsigned* __restrict__ words) {
    const int lane = threadIdx.x & 63;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += (int64_t)gridDim.x * 4) {
        double acc = 0.0;
        int c2 = 0;
        for (int j = lane; j < row_bytes; j += 64) {
            int cs = 0;
            if (j < d) {
                cs = sq_encode1(load_elem(x, r * d + j, x_dt), trained[j], trained[d + j]) - 128;
                const double t = (double)trained[d + j] / 255.0 * (double)cs;
                acc = fma(t, t, acc);
                c2 += cs * cs;
            }
            codes[r * row_bytes + j] = (char)cs;
        }
        acc = wave_sum_f64(acc);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c2 += __shfl_xor(c2, o, 64);
        if (lane == 0) {
            const float f = (float)acc;
            nc[r] = f;
            atomicMax(words + SQ_W_MAXNC, __float_as_uint(f));  // (non-negative floats order as uints)
            atomicMax(words + SQ_W_MAXC2, (unsigned)c2);
        }
    }
}

__global__ __launch_bounds__(SQ_THREADS) void k_sq_encode_u8(const void* __restrict__ x, int x_dt, int64_t n, int d,
                                                             const float* __restrict__ trained,
                                                             uint8_t* __restrict__ out) {
    const int64_t items = n * d;
    for (int64_t e = (int64_t)blockIdx.x * SQ_THREADS + threadIdx.x; e < items; e += (int64_t)gridDim.x * SQ_THREADS) {
        const int j = (int)(e % d);
        out[e] = (uint8_t)sq_encode1(load_elem(x, e, x_dt), trained[j], trained[d + j]);
    }
}

__global__ __launch_bounds__(SQ_THREADS) void k_sq_decode(const char* __restrict__ codes, int stride, int flip,
                                                          int64_t nrows, const int64_t* __restrict__ keys,
                                                          int64_t key0, int64_t n, int d,
                                                          const float* __restrict__ trained, float* __restrict__ out) {
    const int64_t items = n * d;
    for (int64_t e = (int64_t)blockIdx.x * SQ_THREADS + threadIdx.x; e < items; e += (int64_t)gridDim.x * SQ_THREADS) {
        const int64_t i = e / d;
        const int j = (int)(e - i * d);
        const int64_t r = keys ? keys[i] : key0 + i;
        float v = __uint_as_float(0xffffffffu);
        if (r >= 0 && r < nrows) {
            const int cs = (int)(signed char)((unsigned char)codes[r * stride + j] ^ (unsigned char)flip);
            v = sq_decode1(cs, trained[j], trained[d + j]);
        }
        out[e] = v;
    }
}

// ---------------------------------------------------------------------------
// query preparation: one wave per query row of the padded batch.
//
// The scan key of (query, row) is  a = fl(n_c) - 2 sigma fl(S)  (IP: -sigma
// fl(S)) with S = a1 + a2 / 256 + a3 / 65536 the planes' exact integer dots, and
// a + shift estimates the exact key of the DECODED fp32 row y_f = m + s o c' +
// delta (|delta| <= rho_dec, k_sq_consts):
//   L2  D(y_f) + 2 rho_dec sqrt(D(y_f)) >= a + |z|^2 - E,   |a + |z|^2 - D| <= E + 2 rho_dec sqrt(D)
//       E = 2 rho' C + u (2 M^2 + 8 A) + rho_dec^2
//   IP  |a - x.m + x.y_f| <= E = rho' C + 3 u A + |x| rho_dec
// rho' = |w - w_op| (the operand residual; Cauchy-Schwarz against C = sqrt(max
// sum c'^2)), M^2 = max n_c, A = sigma (|h1| + |h2| / 256 + |h3| / 65536) C
// bounds every partial sum of sigma S: forming fl(S) costs two roundings and,
// for d > 1032, the three conversions f32(acc) (3 u A in all, doubled by the
// factor 2 of L2); fl(n_c) and the final addition cost u M^2 and u (M^2 + 2 A).
// There is no accumulation term: the MFMA sums integers.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(SQ_THREADS) void k_sq_prep(SqPrep p) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= p.nq_pad) return;
    if (r == 0 && lane == 0)
        for (int i = 0; i < 2; ++i)
            if (p.zero[i]) *p.zero[i] = 0;
    const bool live = r < p.nq;
    const int rb = p.row_bytes, d = p.d;
    const bool l2 = p.metric == L2;
    double sh = 0.0, xx = 0.0, wmax = 0.0;
    for (int c = lane; c < rb; c += 64) {
        const float v = (live && c < d) ? load_elem(p.q, r * d + c, p.q_dt) : 0.0f;
        p.qf32[r * (int64_t)rb + c] = v;
        if (c < d) {
            double m, s;
            sq_affine(p.trained, d, c, m, s);
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
            const float v = p.qf32[r * (int64_t)rb + c];
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
        p.planes[((int64_t)0 * p.nq_pad + r) * rb + c] = (char)(int)h1;
        p.planes[((int64_t)1 * p.nq_pad + r) * rb + c] = (char)(int)h2;
        p.planes[((int64_t)2 * p.nq_pad + r) * rb + c] = (char)(int)h3;
    }
    h1s = wave_sum_f64(h1s);
    h2s = wave_sum_f64(h2s);
    h3s = wave_sum_f64(h3s);
    res2 = wave_sum_f64(res2);
    if (lane != 0) return;
    p.sigma[r] = (float)sg;
    if (!live) return;
    const double u = 5.9604644775390625e-8;  // 2^-24
    const double C = sqrt((double)p.words[SQ_W_MAXC2]);
    const double M2 = (double)__uint_as_float(p.words[SQ_W_MAXNC]);
    const double rdec = (double)__uint_as_float(p.words[SQ_W_RHO]);
    const double A = sg * (sqrt(h1s) + sqrt(h2s) / 256.0 + sqrt(h3s) / 65536.0) * C;
    const double rp = sqrt(res2);
    double eps;
    if (l2) eps = 2.0 * rp * C + u * (2.0 * M2 + 8.0 * A) * 1.01 + rdec * rdec + 1e-12 * sh;
    else eps = rp * C + 3.0 * u * A * 1.01 + sqrt(xx) * rdec + 1e-12 * fabs(sh);
    p.qeps[r] = bad ? FX_INF : (float)(eps * 1.0625 + 1e-30);
    p.qrho[r] = (float)(rp * 1.0000002);
    p.qshift[r] = l2 ? sh : -sh;
}

// ---------------------------------------------------------------------------
// the scan: scan_tiles_128 with int8 operands.  Per 64-B stage the workgroup
// moves 8 one-KiB pieces of code rows (16 rows x 64 B, lane l: row l & 15, bytes
// 16 (l >> 4) ..) and 24 pieces of the query tile's three planes, 2 + 6 per
// wave; a fragment is the lane's 16 B of its piece for A and B alike, so the k
// order inside the chunk does not matter (as Frag<F32> notes).  Rows at or past
// ntotal are masked by row number (codes 0 and n_c = 0 would look like rows).
// ---------------------------------------------------------------------------
template <int METRIC>
__global__ __launch_bounds__(SCAN_THREADS, 1) void k_sq_scan(SqScan p) {
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
    const int rb = p.row_bytes;
    const int nks = rb / SQ_STAGE_B;
    const int G = (ct1 - ct0) * nks;

    int aoff[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) aoff[j] = ((wave * 2 + j) * 16 + (lane & 15)) * rb + (lane >> 4) * 16;
    int64_t boff[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        const int bi = wave * 6 + j, plane = bi >> 3, qblk = bi & 7;
        boff[j] = ((int64_t)plane * p.nq_pad + q0 + qblk * 16 + (lane & 15)) * rb + (lane >> 4) * 16;
    }
    // the key's scale per query column: -2 sigma (L2), -sigma (IP); a power of two
    float sg[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) sg[n] = (METRIC == L2 ? -2.0f : -1.0f) * p.sigma[q0 + tile_qloc(n)];

    auto issue = [&](int g) {
        const int t = g / nks, ks = g - t * nks;
        char* buf = smem + (g & 1) * SQ_STAGE_BYTES;
        const int64_t row0 = (int64_t)(ct0 + t) * TILE_R;
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
    for (int g = 0; g < G; ++g) {
        if (g + 1 < G) issue(g + 1);
        const char* buf = smem + (g & 1) * SQ_STAGE_BYTES;
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
            // the key, formed here only: n_c - 2 sigma (f32(a1) + f32(a2) / 256 + f32(a3) / 65536)
            auto key = [&](int m, int n, int i) __attribute__((always_inline)) -> float {
                const float s = fmaf((float)acc[2][m][n][i], 1.0f / 65536.0f,
                                     fmaf((float)acc[1][m][n][i], 1.0f / 256.0f, (float)acc[0][m][n][i]));
                return METRIC == L2 ? fmaf(sg[n], s, yn[m][i]) : sg[n] * s;
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
// nl), 16 codes per step
template <int METRIC>
__device__ __forceinline__ double sq_exact_partial(const float* __restrict__ xq, const char* __restrict__ row, int d,
                                                   const float* __restrict__ trained, int sub, int nl) {
    double acc = 0.0;
    for (int c = sub; c * 16 < d; c += nl) {
        const uint4 raw = *(const uint4*)(row + c * 16);
        const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int j = c * 16 + e;
            if (j < d) {
                const int cs = (int)(signed char)((w[e >> 2] >> (8 * (e & 3))) & 0xffu);
                const double y = (double)sq_decode1(cs, trained[j], trained[d + j]);
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

// merge + exact refine + certification: one wave per query (k_refine's three
// phases over the [qtile][split][TILE_Q][KP] lists; no shared threshold, so
// every split pruned only with its own KP-th key)
template <int METRIC>
__global__ __launch_bounds__(256) void k_sq_refine(SqRefine p) {
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

    const float* xq = p.qf32 + q * (int64_t)p.row_bytes;
    const int grp = lane >> 4, sub = lane & 15;
    double ex = 0.0;
    for (int r = 0; r < KP / 4; ++r) {
        const int row = __shfl(bi, r * 4 + grp, 64);
        double a = 0.0;
        if (row != INT_MAX)
            a = sq_exact_partial<METRIC>(xq, p.codes + (int64_t)row * p.row_bytes, p.d, p.trained, sub, 16);
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
        const double rho = METRIC == L2 ? (double)__uint_as_float(p.words[SQ_W_RHO]) : 0.0;
        flagq = !sq_certified(kth, td, p.qshift[q], p.qeps[q], rho);
    }
    if (flagq && lane == 0) {
        const int pos = atomicAdd(p.n_flag, 1);
        p.n_flag[1 + pos] = (int)q;
    }
}

// ---------------------------------------------------------------------------
// the exact path (k_ivf_exact / k_ivf_merge over the whole index in xs splits)
// ---------------------------------------------------------------------------
template <int METRIC>
__global__ __launch_bounds__(BT_THREADS) void k_sq_exact(SqExact p) {
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
        const float* xq = p.qf32 + q * p.row_bytes;
        const int64_t a = p.ntotal * c / p.xs, b = p.ntotal * (c + 1) / p.xs;
        bt_init(&st);
        for (int64_t base = a; base < b; base += BT_THREADS) {
            const int64_t row = base + threadIdx.x;
            const bool valid = row < b;
            float key = FX_INF;
            if (valid) {
                const double v = sq_exact_partial<METRIC>(xq, p.codes + row * p.row_bytes, p.d, p.trained, 0, 1);
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
__global__ __launch_bounds__(BT_THREADS) void k_sq_merge(SqExact p) {
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
hipError_t launch_sq_minmax_reset(unsigned* mm, int d, unsigned long long* bad, hipStream_t s) {
    hipLaunchKernelGGL(k_sq_minmax_reset, dim3(sq_grid(2 * (int64_t)d, SQ_THREADS)), dim3(SQ_THREADS), 0, s, mm, d, bad);
    return hipGetLastError();
}

hipError_t launch_sq_minmax(const void* x, int x_dt, int64_t n, int d, unsigned* mm, unsigned long long* bad,
                            hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sq_minmax, dim3(std::min<unsigned>(1024u, sq_grid(n, 32))), dim3(SQ_THREADS), 0, s, x, x_dt, n,
                       d, mm, bad);
    return hipGetLastError();
}

hipError_t launch_sq_finish(const unsigned* mm, int d, int uniform, float* trained, hipStream_t s) {
    hipLaunchKernelGGL(k_sq_finish, dim3(1), dim3(SQ_THREADS), 0, s, mm, d, uniform, trained);
    return hipGetLastError();
}

hipError_t launch_sq_consts(const float* trained, int d, unsigned* words, hipStream_t s) {
    hipLaunchKernelGGL(k_sq_consts, dim3(1), dim3(SQ_THREADS), 0, s, trained, d, words);
    return hipGetLastError();
}

hipError_t launch_sq_encode(const void* x, int x_dt, int64_t n, int d, const float* trained, int row_bytes,
                            char* codes_row0, float* nc_row0, unsigned* words, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sq_encode, dim3(sq_grid(n, 4)), dim3(SQ_THREADS), 0, s, x, x_dt, n, d, trained, row_bytes,
                       codes_row0, nc_row0, words);
    return hipGetLastError();
}

hipError_t launch_sq_encode_u8(const void* x, int x_dt, int64_t n, int d, const float* trained, uint8_t* out,
                               hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sq_encode_u8, dim3(sq_grid(n * d, SQ_THREADS)), dim3(SQ_THREADS), 0, s, x, x_dt, n, d, trained,
                       out);
    return hipGetLastError();
}

hipError_t launch_sq_decode(const char* codes, int stride, int flip, int64_t nrows, const int64_t* keys, int64_t key0,
                            int64_t n, int d, const float* trained, float* out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_sq_decode, dim3(sq_grid(n * d, SQ_THREADS)), dim3(SQ_THREADS), 0, s, codes, stride, flip, nrows,
                       keys, key0, n, d, trained, out);
    return hipGetLastError();
}

hipError_t launch_sq_prep(const SqPrep& p, hipStream_t s) {
    if (p.nq_pad <= 0 || p.nq_pad % TILE_Q != 0 || p.row_bytes % ROW_ALIGN != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_sq_prep, dim3((unsigned)((p.nq_pad + 3) / 4)), dim3(SQ_THREADS), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_sq_scan(int metric, const SqScan& p, hipStream_t s) {
    if (p.row_bytes <= 0 || p.row_bytes % ROW_ALIGN != 0 || p.n_qtiles <= 0 || p.splits <= 0 ||
        p.splits > p.n_ctiles || (int64_t)p.n_qtiles * TILE_Q > p.nq_pad ||
        (int64_t)p.n_qtiles * p.splits > (int64_t)INT32_MAX || (int64_t)p.n_ctiles * TILE_R < p.ntotal)
        return hipErrorInvalidValue;
    const int grid = p.n_qtiles * p.splits;
    if (metric == L2) return launch_with_lds(k_sq_scan<L2>, grid, SCAN_THREADS, LDS_SCAN_BYTES, s, p);
    return launch_with_lds(k_sq_scan<IP>, grid, SCAN_THREADS, LDS_SCAN_BYTES, s, p);
}

hipError_t launch_sq_refine(int metric, const SqRefine& p, hipStream_t s) {
    if (p.nq <= 0 || p.k <= 0 || p.k > KP || p.splits <= 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.nq + 3) / 4));
    if (metric == L2) hipLaunchKernelGGL(k_sq_refine<L2>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(k_sq_refine<IP>, grid, dim3(256), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_sq_exact(int metric, const SqExact& p, hipStream_t s) {
    if (p.k <= 0 || p.k > FX_BIG_K || p.xs <= 0) return hipErrorInvalidValue;
    if (metric == L2) {
        hipLaunchKernelGGL(k_sq_exact<L2>, dim3(SQ_EXACT_GRID), dim3(BT_THREADS), 0, s, p);
        hipLaunchKernelGGL(k_sq_merge<L2>, dim3(SQ_MERGE_GRID), dim3(BT_THREADS), 0, s, p);
    } else {
        hipLaunchKernelGGL(k_sq_exact<IP>, dim3(SQ_EXACT_GRID), dim3(BT_THREADS), 0, s, p);
        hipLaunchKernelGGL(k_sq_merge<IP>, dim3(SQ_MERGE_GRID), dim3(BT_THREADS), 0, s, p);
    }
    return hipGetLastError();
}

}  // namespace fx

// fx_sq_common.h -- device helpers the two 8-bit indexes share (fx_sq.hip, fx_ivfsq.hip; fx_pq.hip
// and fx_ivfpq.hip take the certification test, fx_ivfpq.hip the rounded addition too): the
// codec's scalar encode / decode, the affine form of a table entry, the digit of a query
// operand plane, the refine's certification test, and the stage layout of the int8 tile loop.
#pragma once
#include "fx_device.h"

namespace fx {

// the int8 scans' LDS: k_scan_topk's carve; its 64 KiB double buffer holds two
// stages of (128 code rows + 3 x 128 plane rows) x 64 B
constexpr int SQ_STAGE_BYTES = (TILE_R + SQ_P * TILE_Q) * SQ_STAGE_B;
static_assert(2 * SQ_STAGE_BYTES == LDS_STAGE, "the int8 stages fill k_scan_topk's double buffer");

typedef int i32x4 __attribute__((ext_vector_type(4)));

// one rounded fp32 addition / subtraction that no neighbouring multiply is fused into
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

// the decoded value of signed code cs: two rounded fp32 operations on the
// table value (c + 0.5) / 255, bitwise a numpy fp32 expression
__device__ __forceinline__ float sq_decode1(int cs, float vmin, float vdiff) {
    // contraction off, plain operators: each is one correctly rounded fp32 operation (hipcc's default
    // fp32 division is correctly rounded), where the compiler would otherwise fuse the multiply into the add
#pragma clang fp contract(off)
    const float t = ((float)(cs + 128) + 0.5f) / 255.f;
    const float p = t * vdiff;
    return vmin + p;
}
// the unsigned code of x (each operation rounded once, no contraction)
__device__ __forceinline__ int sq_encode1(float x, float vmin, float vdiff) {
#pragma clang fp contract(off)
    float xi = 0.f;
    if (vdiff != 0.f) {
        const float num = x - vmin;
        xi = num / vdiff;
        xi = xi > 0.f ? (xi < 1.f ? xi : 1.f) : 0.f;  // (NaN -> 0)
    }
    const float sc = 255.f * xi;
    return (int)sc;
}
// y = m + s c' in exact arithmetic: the scale and the box centre of dimension j
__device__ __forceinline__ void sq_affine(const float* __restrict__ trained, int d, int j, double& m, double& s) {
    s = (double)trained[d + j] / 255.0;
    m = (double)trained[j] + 128.5 * s;
}

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double sq_digit(double r) {
    const double h = rint(r);
    return h > 127.0 ? 127.0 : h < -127.0 ? -127.0 : h;
}

// k_refine's certification (fx_kernels.hip certified_v): every row the
// selection dropped has scan key >= tb, so its exact distance D satisfies
// D + 2 rho sqrt(D) >= T = tb + shift - E (rho = rho_dec for L2, 0 for IP)
__device__ __forceinline__ bool sq_certified(float kth, float tb, double shift, float eps, double rho) {
    const double T = (double)tb + shift - (double)eps;
    double dmin = T;
    if (rho > 0.0) {
        const double t = T > 0.0 ? T : 0.0;
        const double sd = t / (sqrt(rho * rho + t) + rho);
        dmin = sd * sd * (1.0 - 1e-12);
    }
    const double kup = (double)kth + fabs((double)kth) * 2.384185791015625e-7;  // + 2 ulp
    return kup < dmin;
}

}  // namespace fx

// Tile shape, operand split and MFMA half step shared by the backbone forward (backbone.hip) and backward
// (backbone_backward.hip) implicit-GEMM kernels.
#pragma once

#include "common.h"

namespace sdetr {
namespace {

constexpr int kBM = 256, kBN = 128, kBK = 32, kBThreads = 512;
constexpr int kBRow32 = kBK * 4 + 16;   // bytes per fp32 activation row in LDS (144)
constexpr int kBRow16 = kBK * 2 + 16;   // bytes per 16-bit row in LDS (80)
constexpr int kBPlane = kBN * kBRow16;  // 10 240: one weight plane
constexpr int kBMaxImages = 64;

template <bool X3>
struct BCfg {
    static constexpr int kA = kBM * (X3 ? kBRow32 : kBRow16);   // 36 864 | 20 480
    static constexpr int kB = (X3 ? 3 : 1) * kBPlane;           // 30 720 | 10 240
    static constexpr int kStage = kA + kB;
    static constexpr int kLds = 2 * kStage;                     // 135 168 | 61 440
};

typedef __bf16 b_bf16x8_t __attribute__((ext_vector_type(8)));
typedef float b_f32x16_t __attribute__((ext_vector_type(16)));

__device__ __forceinline__ int b_acc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }
__device__ __forceinline__ uint32_t b_off(bool ok, uint32_t off) { return ok ? off : 0xfffffff0u; }
__device__ __forceinline__ uint32_t b_pack_hi(float lo, float hi)
{
    return __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo), 0x07060302u);
}
struct BFrag3 {
    u32x4_t p[3];
};
// exact three-way bf16 split of 8 fp32 values (truncation), as gemm_x3.hip / frontend.hip
__device__ __forceinline__ BFrag3 b_split(const float4 lo, const float4 hi)
{
    const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    float r1[8], r2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        r1[i] = x[i] - __uint_as_float(__float_as_uint(x[i]) & 0xffff0000u);
        r2[i] = r1[i] - __uint_as_float(__float_as_uint(r1[i]) & 0xffff0000u);
    }
    BFrag3 f;
    f.p[0] = u32x4_t{b_pack_hi(x[0], x[1]), b_pack_hi(x[2], x[3]), b_pack_hi(x[4], x[5]), b_pack_hi(x[6], x[7])};
    f.p[1] = u32x4_t{b_pack_hi(r1[0], r1[1]), b_pack_hi(r1[2], r1[3]), b_pack_hi(r1[4], r1[5]), b_pack_hi(r1[6], r1[7])};
    f.p[2] = u32x4_t{b_pack_hi(r2[0], r2[1]), b_pack_hi(r2[2], r2[3]), b_pack_hi(r2[4], r2[5]), b_pack_hi(r2[6], r2[7])};
    return f;
}
__device__ __forceinline__ b_f32x16_t b_mfma_bf16(u32x4_t a, u32x4_t b, b_f32x16_t c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(b_bf16x8_t, a), __builtin_bit_cast(b_bf16x8_t, b), c, 0,
                                                   0, 0);
}

// one half step (16 reduction indices) of a wave's 64 x 64 tile
template <bool X3>
__device__ __forceinline__ void half_step(const char *fa, const char *fb, int kk, b_f32x16_t (&acc)[2][2])
{
    if (X3) {
        BFrag3 a[2], b[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const float4 *qa = reinterpret_cast<const float4 *>(fa + t * 32 * kBRow32 + kk * 64);
            a[t] = b_split(qa[0], qa[1]);
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                b[t].p[pl] = *reinterpret_cast<const u32x4_t *>(fb + t * 32 * kBRow16 + pl * kBPlane + kk * 32);
        }
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                b_f32x16_t c = acc[rt][ct];
                c = b_mfma_bf16(a[rt].p[2], b[ct].p[0], c);   // smallest terms first
                c = b_mfma_bf16(a[rt].p[0], b[ct].p[2], c);
                c = b_mfma_bf16(a[rt].p[1], b[ct].p[1], c);
                c = b_mfma_bf16(a[rt].p[1], b[ct].p[0], c);
                c = b_mfma_bf16(a[rt].p[0], b[ct].p[1], c);
                c = b_mfma_bf16(a[rt].p[0], b[ct].p[0], c);
                acc[rt][ct] = c;
            }
    } else {
        uint4 a[2], b[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            a[t] = *reinterpret_cast<const uint4 *>(fa + t * 32 * kBRow16 + kk * 32);
            b[t] = *reinterpret_cast<const uint4 *>(fb + t * 32 * kBRow16 + kk * 32);
        }
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = mfma_act_32x32x16(a[rt], b[ct], acc[rt][ct]);
    }
}

}  // namespace
}  // namespace sdetr

// What the row-stream backbones (convnext.hip, focalnet.hip, swin.hip) share on top of backbone_conv_core.h: the LayerNorm
// over the channels of fp32 rows (one wave per row, the row in registers), the host checks of a rows op, the dispatch of
// the implicit-GEMM kernel over precision and input layout; with plan.h, the bodies of a family's three plan entry points.
#pragma once

#include "backbone_conv_core.h"
#include "plan.h"

namespace sdetr {
namespace {

constexpr int kRowThreads = 256;              // four rows per workgroup
constexpr int kRowMaxC = 3072;                // the widest row: kRowQuads quads per lane
constexpr int kRowQuads = kRowMaxC / 256;

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// a row held by one wave, quad lane + 64 i in v[i] (quads past nq are zeros and do not count), and its statistics
struct LnRow {
    float4 v[kRowQuads];
    float mean, rstd;
};

__device__ __forceinline__ void ln_row_load(const float *row, int nq, int lane, LnRow &r)
{
#pragma unroll
    for (int i = 0; i < kRowQuads; ++i) {
        const int q = lane + 64 * i;
        r.v[i] = q < nq ? *reinterpret_cast<const float4 *>(row + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// mean, then the variance about it
__device__ __forceinline__ void ln_row_stats(int nq, int lane, float inv_c, float eps, LnRow &r)
{
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kRowQuads; ++i) s += (r.v[i].x + r.v[i].y) + (r.v[i].z + r.v[i].w);
    r.mean = wave_sum(s) * inv_c;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < kRowQuads; ++i) {
        if (lane + 64 * i >= nq) continue;
        const float dx = r.v[i].x - r.mean, dy = r.v[i].y - r.mean, dz = r.v[i].z - r.mean, dw = r.v[i].w - r.mean;
        ss += (dx * dx + dy * dy) + (dz * dz + dw * dw);
    }
    r.rstd = 1.f / sqrtf(wave_sum(ss) * inv_c + eps);
}

// the normalised row (+ res, an fp32 row, or null) to out (fp32 or compute dtype) and to out16 (a 16-bit copy, or null)
template <bool F32OUT>
__device__ __forceinline__ void ln_row_write(const LnRow &r, const float *gamma, const float *beta, const float *res, int nq,
                                             int lane, char *out, uint16_t *out16)
{
#pragma unroll
    for (int i = 0; i < kRowQuads; ++i) {
        const int q = lane + 64 * i;
        if (q >= nq) continue;
        const float4 g = *reinterpret_cast<const float4 *>(gamma + 4 * q);
        const float4 be = *reinterpret_cast<const float4 *>(beta + 4 * q);
        float o0 = fmaf((r.v[i].x - r.mean) * r.rstd, g.x, be.x), o1 = fmaf((r.v[i].y - r.mean) * r.rstd, g.y, be.y);
        float o2 = fmaf((r.v[i].z - r.mean) * r.rstd, g.z, be.z), o3 = fmaf((r.v[i].w - r.mean) * r.rstd, g.w, be.w);
        if (res) {
            const float4 b = *reinterpret_cast<const float4 *>(res + 4 * q);
            o0 += b.x, o1 += b.y, o2 += b.z, o3 += b.w;
        }
        if (F32OUT) *reinterpret_cast<float4 *>(out + (int64_t)q * 16) = make_float4(o0, o1, o2, o3);
        else *reinterpret_cast<uint2 *>(out + (int64_t)q * 8) = make_uint2(pack_act2(o0, o1), pack_act2(o2, o3));
        if (out16) *reinterpret_cast<uint2 *>(out16 + 4 * q) = make_uint2(pack_act2(o0, o1), pack_act2(o2, o3));
    }
}

// out = (res +) LayerNorm(x) over C of fp32 rows [rows][C]; out fp32 or compute dtype, out16 (or null) a 16-bit copy
template <bool F32OUT>
__global__ void __launch_bounds__(kRowThreads) ln_rows_kernel(const float *x, const float *gamma, const float *beta,
                                                              const float *res, int64_t rows, int c, float eps, char *out,
                                                              uint16_t *out16)
{
    const int lane = threadIdx.x & 63, nq = c >> 2;
    const int64_t stride = (int64_t)gridDim.x * (kRowThreads / 64);
    for (int64_t r = (int64_t)blockIdx.x * (kRowThreads / 64) + (threadIdx.x >> 6); r < rows; r += stride) {
        LnRow row;
        ln_row_load(x + r * c, nq, lane, row);
        ln_row_stats(nq, lane, 1.f / (float)c, eps, row);
        ln_row_write<F32OUT>(row, gamma, beta, res ? res + r * c : nullptr, nq, lane, out + r * c * (F32OUT ? 4 : 2),
                             out16 ? out16 + r * c : nullptr);
    }
}

// ------------------------------------------------------------------------------------------------------------ host
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
template <class... P>
bool all_aligned16(const P *...p)
{
    return (aligned16(p) && ...);
}

// precision and the size of a rows op's input [batch, h, w, c]
inline int check_rows_shape(const char *what, int batch, int h, int w, int c, int precision)
{
    if (precision != 0 && precision != 1) return fail("%s: precision must be 0 or 1", what);
    if (batch < 1 || h < 1 || w < 1 || c < 1) return fail("%s: bad shape (batch %d, %d x %d, channels %d)", what, batch, h, w, c);
    if ((int64_t)batch * h * w * c >= (int64_t(1) << 29)) return fail("%s: tensors too large for 32-bit offsets", what);
    return 0;
}

// a row-LayerNorm op: the shape, a width the register row holds, the four tensors every family has
inline int check_ln_rows(const char *what, int batch, int h, int w, int c, int precision, const void *x, const float *gamma,
                         const float *beta, const void *out)
{
    if (int rc = check_rows_shape(what, batch, h, w, c, precision)) return rc;
    if (c % 32 || c > kRowMaxC) return fail("%s: channels must be a multiple of 32 up to %d (got %d)", what, kRowMaxC, c);
    if (!x || !gamma || !beta || !out) return fail("%s: null tensor", what);
    if (!all_aligned16(x, gamma, beta, out)) return fail("%s: tensors must be 16-byte aligned", what);
    return 0;
}

inline void launch_ln_rows(hipStream_t s, bool f32out, const void *x, const float *gamma, const float *beta, const float *res,
                           int64_t rows, int c, float eps, void *out, void *out16)
{
    const unsigned blocks = (unsigned)std::min<int64_t>((rows + 3) / 4, 16384);
    const float *xf = reinterpret_cast<const float *>(x);
    char *o = reinterpret_cast<char *>(out);
    uint16_t *o16 = reinterpret_cast<uint16_t *>(out16);
    if (f32out)
        hipLaunchKernelGGL(ln_rows_kernel<true>, dim3(blocks), dim3(kRowThreads), 0, s, xf, gamma, beta, res, rows, c, eps, o, o16);
    else
        hipLaunchKernelGGL(ln_rows_kernel<false>, dim3(blocks), dim3(kRowThreads), 0, s, xf, gamma, beta, res, rows, c, eps, o, o16);
}

template <int EPI>
void launch_rows_gemm(hipStream_t s, const BConv &c, bool x3)
{
    if (x3) launch_conv<true, false, EPI>(s, c);
    else launch_conv<false, false, EPI>(s, c);
}

template <int EPI>
void launch_gemm(hipStream_t s, const BConv &c, bool x3, bool nchw)
{
    if (!nchw) launch_rows_gemm<EPI>(s, c, x3);
    else if (x3) launch_conv<true, true, EPI>(s, c);
    else launch_conv<false, true, EPI>(s, c);
}

}  // namespace
}  // namespace sdetr

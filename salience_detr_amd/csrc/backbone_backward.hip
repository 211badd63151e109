// The backbone's training backward (row N0, DESIGN.md §4 "Backbone"): the gradients of the ops backbone.hip runs forward,
// y = relu?(conv(x, w') + b' (+ residual)) with w' = w * s[co], s = gamma / sqrt(var + eps) (FrozenBatchNorm2d folded).
// `dz` is the gradient at an op's pre-activation, channels-last [B, Ho, Wo, co] in the compute dtype.
//
//   backbone_dgrad_pack_kernel  w' in the backward-data reduction order k = (ky * ks + kx) * co32 + co (co32 = co rounded
//                               up to 32, zero columns past co), planes [pl][ci][ks * ks * co32] as backbone_pack_kernel
//                               splits them; also s[co]
//   backbone_dgrad_kernel       dx[pixel, ci] = sum_{tap, co} dz[pixel @ tap, co] w'[co, tap, ci]: the forward's implicit
//                               GEMM (same tile, same half step) with the INPUT pixels as rows.  Stride 2 is decomposed by
//                               input parity: grid.z enumerates the stride^2 parity classes, each with the fixed subset of
//                               taps that reach it (3x3: 1, 2, 2, 4 taps; 1x1: one class with its tap, three with none,
//                               which only write the epilogue), so no zero is multiplied.  Epilogue
//                               out = (acc (+ add)) * (mask > 0)?: `add` is the gradient another consumer of the same
//                               tensor has produced, `mask` the producer's stored output (its ReLU backward).
//   backbone_wgrad_kernel       dw[co, (tap, ci)] = s[co] sum_pixel dz[pixel, co] x[pixel @ tap, ci]: 128 x 128 tiles, one
//                               tap per tile column, 32 pixels per step.  Both operands have the pixel as their slow
//                               index in memory: they are TRANSPOSED ON THE WAY INTO LDS (16-byte global loads, 4-byte
//                               LDS stores at [channel][pixel]: an fp32 word, or two adjacent pixels' 16-bit values packed)
//                               so the MFMA fragments are read as 16-byte rows exactly as the forward reads them.
//                               fp32: both operands are split three ways fragment by fragment (six products).
//   backbone_*_reduce_kernel    the reduction split over workgroups: pieces summed in split order (no atomics), then the
//                               epilogue.
//   backbone_ingest_kernel      a returned stage's cotangent, fp32 NCHW -> channels-last dz (+ add) * (mask > 0)
// Every kernel writes every element of its output: a capture holds no memset node.
#include <algorithm>

#include "backbone_core.h"
#include "common.h"
#include "plan.h"

namespace sdetr {
namespace {

constexpr int kWM = 128, kWN = 128, kWK = 32, kWThreads = 256;   // the wgrad tile: co x ci x pixels

struct BDgrad {
    const char *dz;         // [B, Ho, Wo, co] compute dtype
    const uint16_t *w;      // packed [planes][ci][ks * ks * cop]
    const char *add;        // [B, H, W, ci] compute dtype, or null
    const char *mask;       // [B, H, W, ci] compute dtype, or null
    char *out;              // [B, H, W, ci] compute dtype
    float *partial;         // [splits][M][ci]
    uint32_t dz_bytes, w_bytes;
    int batch, ci, h, w_in, co, cop, ks, stride, pad, ho, wo, M, kfull, splits;
    int64_t plane;          // ci * kfull
};

struct BWgrad {
    const char *dz;         // [M, co] compute dtype
    const char *x;          // [B, H, W, ci] compute dtype
    const float *scale;     // [co]
    float *out;             // f32 [co, ci, ks, ks]
    float *partial;         // [splits][co][ks * ks][ci]
    uint32_t dz_bytes, x_bytes;
    int batch, ci, h, w_in, co, ks, stride, pad, ho, wo, M, splits, steps_per_split;
};

template <bool X3>
__device__ __forceinline__ float load_act(const char *p, int64_t e)
{
    if (X3) return reinterpret_cast<const float *>(p)[e];
    return act_lo(reinterpret_cast<const uint16_t *>(p)[e]);
}
template <bool X3>
__device__ __forceinline__ void store_act(char *p, int64_t e, float v)
{
    if (X3) reinterpret_cast<float *>(p)[e] = v;
    else reinterpret_cast<uint16_t *>(p)[e] = (uint16_t)f32_to_act_bits(v);
}

// ------------------------------------------------------------------------------------------------------------ dgrad
// the taps of one axis that reach input parity `par`: (par + pad - k) a multiple of the stride (ks <= 3: at most 2)
__device__ __forceinline__ int axis_taps(int par, int pad, int ks, int stride, int &t0, int &t1)
{
    int n = 0;
    t0 = t1 = 0;
    for (int k = 0; k < ks; ++k) {
        if (stride == 2 && ((par + pad - k) & 1)) continue;
        if (n == 0) t0 = k;
        else if (n == 1) t1 = k;
        ++n;
    }
    return n;   // stride 1: ks taps -- handled by the caller (t0/t1 unused there)
}

struct DClass {
    int py, px, hc, wc, Mc, nty, ntx, ty0, ty1, tx0, tx1, steps;
};
__device__ __forceinline__ DClass dgrad_class(const BDgrad &c, int cls)
{
    DClass d;
    d.py = cls / c.stride;
    d.px = cls - d.py * c.stride;
    d.hc = (c.h - d.py + c.stride - 1) / c.stride;
    d.wc = (c.w_in - d.px + c.stride - 1) / c.stride;
    d.Mc = c.batch * d.hc * d.wc;
    if (c.stride == 1) {
        d.nty = d.ntx = c.ks;
        d.ty0 = d.ty1 = d.tx0 = d.tx1 = 0;
    } else {
        d.nty = axis_taps(d.py, c.pad, c.ks, c.stride, d.ty0, d.ty1);
        d.ntx = axis_taps(d.px, c.pad, c.ks, c.stride, d.tx0, d.tx1);
    }
    d.steps = d.nty * d.ntx * (c.cop / kBK);
    return d;
}
// (ky, kx) of the class's tap number t
__device__ __forceinline__ void class_tap(const BDgrad &c, const DClass &d, int t, int &ky, int &kx)
{
    const int a = t / d.ntx, b = t - a * d.ntx;
    if (c.stride == 1) {
        ky = a;
        kx = b;
    } else {
        ky = a ? d.ty1 : d.ty0;
        kx = b ? d.tx1 : d.tx0;
    }
}

// input pixel of class row mc: (iy + pad, ix + pad), the image's first dz pixel and the pixel's own index in dx
struct DRow {
    int ny, nx, base, g;
};
__device__ __forceinline__ DRow dgrad_row(const BDgrad &c, const DClass &d, int mc)
{
    DRow r;
    if (mc >= d.Mc) {
        r.ny = -(1 << 28);   // every tap out of range: the row reads zeros
        r.nx = 0;
        r.base = 0;
        r.g = -1;
        return r;
    }
    const int hw = d.hc * d.wc, n = mc / hw, rem = mc - n * hw, yc = rem / d.wc, xc = rem - yc * d.wc;
    const int iy = yc * c.stride + d.py, ix = xc * c.stride + d.px;
    r.ny = iy + c.pad;
    r.nx = ix + c.pad;
    r.base = n * c.ho * c.wo;
    r.g = (n * c.h + iy) * c.w_in + ix;
    return r;
}

// A tile: dz rows at one tap, 32 contiguous output channels (zero past co); pieces as the forward's ALoadNHWC
template <bool X3>
struct DLoadA {
    static constexpr int kRows = X3 ? 4 : 2, kStep = X3 ? 64 : 128, kShift = X3 ? 3 : 2, kEsz = X3 ? 4 : 2;
    static constexpr int kPer = X3 ? 4 : 8;   // channels per 16-byte piece
    DRow ri[kRows];
    uint4 v[kRows];
    __device__ __forceinline__ void init(const BDgrad &c, const DClass &d, int m0, int tid)
    {
#pragma unroll
        for (int j = 0; j < kRows; ++j) ri[j] = dgrad_row(c, d, m0 + (tid >> kShift) + kStep * j);
    }
    __device__ __forceinline__ void load(const BDgrad &c, __amdgpu_buffer_rsrc_t rs, int ky, int kx, int c0, bool kok, int tid)
    {
        const int sub = tid & ((1 << kShift) - 1), sh = c.stride - 1;
        const bool cok = kok && c0 + kPer * sub < c.co;
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const int qy = ri[j].ny - ky, qx = ri[j].nx - kx, oy = qy >> sh, ox = qx >> sh;
            const bool ok = cok && qy >= 0 && qx >= 0 && oy < c.ho && ox < c.wo;
            const uint32_t pix = (uint32_t)ri[j].base + (uint32_t)oy * (uint32_t)c.wo + (uint32_t)ox;   // (wraps when !ok)
            v[j] = buffer_load16(rs, b_off(ok, (pix * (uint32_t)c.co + (uint32_t)c0) * kEsz + 16u * (uint32_t)sub));
        }
    }
    __device__ __forceinline__ void store(char *tile, int tid) const
    {
        constexpr int row = X3 ? kBRow32 : kBRow16;
        char *d = tile + (tid >> kShift) * row + 16 * (tid & ((1 << kShift) - 1));
#pragma unroll
        for (int j = 0; j < kRows; ++j) *reinterpret_cast<uint4 *>(d + kStep * j * row) = v[j];
    }
};

// B tile: 128 input channels x 32 reduction indices per plane
template <int PL>
struct DLoadW {
    uint4 q[PL];
    __device__ __forceinline__ void load(const BDgrad &c, __amdgpu_buffer_rsrc_t rs, int n0, int k, bool kok, int tid)
    {
        const int r = n0 + (tid >> 2);
        const bool ok = kok && r < c.ci;
        const uint32_t o = ((uint32_t)r * (uint32_t)c.kfull + (uint32_t)(k + 8 * (tid & 3))) * 2u, plane = (uint32_t)(c.plane * 2);
#pragma unroll
        for (int pl = 0; pl < PL; ++pl) q[pl] = buffer_load16(rs, b_off(ok, o + pl * plane));
    }
    __device__ __forceinline__ void store(char *tile, int tid) const
    {
        char *d = tile + (tid >> 2) * kBRow16 + 16 * (tid & 3);
#pragma unroll
        for (int pl = 0; pl < PL; ++pl) *reinterpret_cast<uint4 *>(d + pl * kBPlane) = q[pl];
    }
};

// out = (v (+ add)) * (mask > 0)?
template <bool X3>
__device__ __forceinline__ void dgrad_emit(const BDgrad &c, int64_t e, float v)
{
    if (c.add) v += load_act<X3>(c.add, e);
    if (c.mask && !(load_act<X3>(c.mask, e) > 0.f)) v = 0.f;
    store_act<X3>(c.out, e, v);
}

template <bool X3>
__global__ void __launch_bounds__(kBThreads, 1) backbone_dgrad_kernel(BDgrad c)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    using Cfg = BCfg<X3>;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int cls = blockIdx.z / c.splits, split = blockIdx.z - cls * c.splits;
    const DClass d = dgrad_class(c, cls);
    const int m0 = blockIdx.x * kBM, n0 = blockIdx.y * kBN;
    if (m0 >= d.Mc) return;   // (uniform: the grid is sized for the largest class)
    const int per = (d.steps + c.splits - 1) / c.splits;
    const int sbeg = min(d.steps, split * per), send = min(d.steps, sbeg + per);
    const int cpt = c.cop / kBK;   // steps per tap
    const __amdgpu_buffer_rsrc_t rx = make_uniform_rsrc(c.dz, c.dz_bytes);
    const __amdgpu_buffer_rsrc_t rw = make_uniform_rsrc(reinterpret_cast<const char *>(c.w), c.w_bytes);

    b_f32x16_t acc[2][2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[rt][ct][i] = 0.f;

    DLoadA<X3> ta;
    DLoadW<X3 ? 3 : 1> tb;
    ta.init(c, d, m0, tid);
    auto fetch = [&](int st) {
        const bool kok = st < send;
        const int t = st / cpt, c0 = (st - t * cpt) * kBK;
        int ky, kx;
        class_tap(c, d, kok ? t : 0, ky, kx);
        ta.load(c, rx, ky, kx, c0, kok, tid);
        tb.load(c, rw, n0, (ky * c.ks + kx) * c.cop + c0, kok, tid);
    };
    if (sbeg < send) {
        fetch(sbeg);
        ta.store(lds, tid);
        tb.store(lds + Cfg::kA, tid);
    }
    __syncthreads();
    const int fa = X3 ? (64 * wm + (lane & 31)) * kBRow32 + (lane >> 5) * 32 : (64 * wm + (lane & 31)) * kBRow16 + (lane >> 5) * 16;
    const int fb = Cfg::kA + (64 * wn + (lane & 31)) * kBRow16 + (lane >> 5) * 16;
    int cur = 0;
    for (int st = sbeg; st < send; ++st) {
        const bool more = st + 1 < send;   // (uniform)
        if (more) fetch(st + 1);
        const char *s = lds + cur * Cfg::kStage;
        half_step<X3>(s + fa, s + fb, 0, acc);
        half_step<X3>(s + fa, s + fb, 1, acc);
        if (more) {
            char *dst = lds + (cur ^ 1) * Cfg::kStage;
            ta.store(dst, tid);
            tb.store(dst + Cfg::kA, tid);
        }
        __syncthreads();
        cur ^= 1;
    }

#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const DRow r = dgrad_row(c, d, m0 + 64 * wm + 32 * rt + b_acc_row(i, lane));
            if (r.g < 0) continue;
#pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
                const int ci = n0 + 64 * wn + 32 * ct + (lane & 31);
                if (ci >= c.ci) continue;
                if (c.splits > 1) c.partial[((int64_t)split * c.M + r.g) * c.ci + ci] = acc[rt][ct][i];
                else dgrad_emit<X3>(c, (int64_t)r.g * c.ci + ci, acc[rt][ct][i]);
            }
        }
}

template <bool X3>
__global__ void __launch_bounds__(256) backbone_dgrad_reduce_kernel(BDgrad c)
{
    const int64_t total = (int64_t)c.M * c.ci, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        float v = c.partial[e];
        for (int z = 1; z < c.splits; ++z) v += c.partial[(int64_t)z * total + e];
        dgrad_emit<X3>(c, e, v);
    }
}

// planes [pl][ci][ks * ks * cop], k = tap * cop + co, zero for co past the end; scale[co] = gamma / sqrt(var + eps).
// `out` null: only the scale.
__global__ void __launch_bounds__(256) backbone_dgrad_pack_kernel(const float *w, const float *gamma, const float *var,
                                                                  float eps, int co, int ci, int ks, int cop, int precision,
                                                                  uint16_t *out, float *scale)
{
    const int kk2 = ks * ks, kfull = kk2 * cop;
    const int64_t total = (int64_t)ci * kfull, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        if (e < co) scale[e] = gamma[e] / sqrtf(var[e] + eps);
        if (!out) continue;
        const int i = (int)(e / kfull), k = (int)(e - (int64_t)i * kfull), tap = k / cop, o = k - tap * cop;
        float v = 0.f;
        if (o < co) v = w[((int64_t)o * ci + i) * kk2 + tap] * (gamma[o] / sqrtf(var[o] + eps));
        if (precision == 0) {
            const float r1 = v - __uint_as_float(__float_as_uint(v) & 0xffff0000u);
            const float r2 = r1 - __uint_as_float(__float_as_uint(r1) & 0xffff0000u);
            out[e] = (uint16_t)(__float_as_uint(v) >> 16);
            out[total + e] = (uint16_t)(__float_as_uint(r1) >> 16);
            out[2 * total + e] = (uint16_t)(__float_as_uint(r2) >> 16);
        } else {
            out[e] = (uint16_t)f32_to_act_bits(v);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ wgrad
template <bool X3>
struct WCfg {
    static constexpr int kRow = X3 ? kBRow32 : kBRow16;
    static constexpr int kOp = kWM * kRow;        // one operand tile: 18 432 | 10 240
    static constexpr int kStage = 2 * kOp;
    static constexpr int kLds = 2 * kStage;       // 73 728 | 40 960
};

// the pixels a thread carries into LDS each step: 4 (fp32: 8 j + lane % 8) or 2 adjacent (16-bit: 2 (lane % 16) + j) of
// the step's 32, tracked incrementally as (image, oy, ox)
template <bool X3>
struct WPixels {
    static constexpr int kN = X3 ? 4 : 2;
    int m[kN], n[kN], oy[kN], ox[kN];
    __device__ __forceinline__ void init(const BWgrad &c, int mbeg, int lane)
    {
#pragma unroll
        for (int j = 0; j < kN; ++j) {
            m[j] = mbeg + (X3 ? 8 * j + (lane & 7) : 2 * (lane & 15) + j);
            const int hw = c.ho * c.wo;
            n[j] = m[j] / hw;
            const int rem = m[j] - n[j] * hw;
            oy[j] = rem / c.wo;
            ox[j] = rem - oy[j] * c.wo;
        }
    }
    __device__ __forceinline__ void advance(const BWgrad &c)
    {
#pragma unroll
        for (int j = 0; j < kN; ++j) {
            m[j] += kWK;
            ox[j] += kWK;
            if (ox[j] >= c.wo) {
                const int q = ox[j] / c.wo;
                ox[j] -= q * c.wo;
                oy[j] += q;
                if (oy[j] >= c.ho) {
                    const int q2 = oy[j] / c.ho;
                    oy[j] -= q2 * c.ho;
                    n[j] += q2;
                }
            }
        }
    }
};

// one operand's 32 pixels x 128 channels, transposed into LDS rows [channel][32 pixels]
template <bool X3>
struct WLoad {
    static constexpr int kN = X3 ? 4 : 2;
    uint4 v[kN];
    // pix[j] = the operand's pixel index (or -1: zeros); ch0 = the tile's first channel, C the operand's channel count
    __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t rs, const int (&pix)[kN], int ch0, int C, int tid)
    {
        const int lane = tid & 63, wave = tid >> 6;
        const int ch = ch0 + (X3 ? 32 * wave + 4 * (lane >> 3) : 8 * ((lane >> 4) + 4 * wave));
#pragma unroll
        for (int j = 0; j < kN; ++j) {
            const bool ok = pix[j] >= 0 && ch < C;
            v[j] = buffer_load16(rs, b_off(ok, ((uint32_t)pix[j] * (uint32_t)C + (uint32_t)ch) * (X3 ? 4u : 2u)));
        }
    }
    __device__ __forceinline__ void store(char *tile, int tid) const
    {
        const int lane = tid & 63, wave = tid >> 6;
        if (X3) {
            char *d = tile + (32 * wave + 4 * (lane >> 3)) * kBRow32 + 4 * (lane & 7);
#pragma unroll
            for (int j = 0; j < kN; ++j) {
                const uint32_t u[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
                for (int q = 0; q < 4; ++q) *reinterpret_cast<uint32_t *>(d + q * kBRow32 + 32 * j) = u[q];
            }
        } else {
            char *d = tile + 8 * ((lane >> 4) + 4 * wave) * kBRow16 + 4 * (lane & 15);
            const uint32_t a[4] = {v[0].x, v[0].y, v[0].z, v[0].w}, b[4] = {v[kN - 1].x, v[kN - 1].y, v[kN - 1].z, v[kN - 1].w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                *reinterpret_cast<uint32_t *>(d + (2 * q) * kBRow16) = (a[q] & 0xffffu) | (b[q] << 16);
                *reinterpret_cast<uint32_t *>(d + (2 * q + 1) * kBRow16) = (a[q] >> 16) | (b[q] & 0xffff0000u);
            }
        }
    }
};

// one half step (16 pixels) of a wave's 64 x 64 tile with BOTH operands fp32 rows, split fragment by fragment
__device__ __forceinline__ void half_step_x3x3(const char *fa, const char *fb, int kk, b_f32x16_t (&acc)[2][2])
{
    BFrag3 a[2], b[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const float4 *qa = reinterpret_cast<const float4 *>(fa + t * 32 * kBRow32 + kk * 64);
        const float4 *qb = reinterpret_cast<const float4 *>(fb + t * 32 * kBRow32 + kk * 64);
        a[t] = b_split(qa[0], qa[1]);
        b[t] = b_split(qb[0], qb[1]);
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
}

template <bool X3>
__global__ void __launch_bounds__(kWThreads, 1) backbone_wgrad_kernel(BWgrad c)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    using Cfg = WCfg<X3>;
    constexpr int kN = X3 ? 4 : 2;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int cit = (c.ci + kWN - 1) / kWN, tap = blockIdx.y / cit, ky = tap / c.ks, kx = tap - ky * c.ks;
    const int m0 = blockIdx.x * kWM, n0 = (blockIdx.y - tap * cit) * kWN;
    const int steps = (c.M + kWK - 1) / kWK;
    const int sbeg = min(steps, (int)blockIdx.z * c.steps_per_split), send = min(steps, sbeg + c.steps_per_split);
    const __amdgpu_buffer_rsrc_t rz = make_uniform_rsrc(c.dz, c.dz_bytes);
    const __amdgpu_buffer_rsrc_t rx = make_uniform_rsrc(c.x, c.x_bytes);

    b_f32x16_t acc[2][2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[rt][ct][i] = 0.f;

    WPixels<X3> px;
    WLoad<X3> ta, tb;
    px.init(c, sbeg * kWK, lane);
    auto fetch = [&]() {
        int pz[kN], pi[kN];
#pragma unroll
        for (int j = 0; j < kN; ++j) {
            const int iy = px.oy[j] * c.stride + ky - c.pad, ix = px.ox[j] * c.stride + kx - c.pad;
            const bool in = px.m[j] < c.M;
            pz[j] = in ? px.m[j] : -1;
            pi[j] = in && (unsigned)iy < (unsigned)c.h && (unsigned)ix < (unsigned)c.w_in ? (px.n[j] * c.h + iy) * c.w_in + ix : -1;
        }
        ta.load(rz, pz, m0, c.co, tid);
        tb.load(rx, pi, n0, c.ci, tid);
        px.advance(c);
    };
    if (sbeg < send) {
        fetch();
        ta.store(lds, tid);
        tb.store(lds + Cfg::kOp, tid);
    }
    __syncthreads();
    const int fa = (64 * wm + (lane & 31)) * Cfg::kRow + (lane >> 5) * (X3 ? 32 : 16);
    const int fb = Cfg::kOp + (64 * wn + (lane & 31)) * Cfg::kRow + (lane >> 5) * (X3 ? 32 : 16);
    int cur = 0;
    for (int st = sbeg; st < send; ++st) {
        const bool more = st + 1 < send;   // (uniform)
        if (more) fetch();
        const char *s = lds + cur * Cfg::kStage;
        if (X3) {
            half_step_x3x3(s + fa, s + fb, 0, acc);
            half_step_x3x3(s + fa, s + fb, 1, acc);
        } else {
            half_step<false>(s + fa, s + fb, 0, acc);
            half_step<false>(s + fa, s + fb, 1, acc);
        }
        if (more) {
            char *dst = lds + (cur ^ 1) * Cfg::kStage;
            ta.store(dst, tid);
            tb.store(dst + Cfg::kOp, tid);
        }
        __syncthreads();
        cur ^= 1;
    }

    const int kk2 = c.ks * c.ks;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int ci = n0 + 64 * wn + 32 * ct + (lane & 31);
        if (ci >= c.ci) continue;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int co = m0 + 64 * wm + 32 * rt + b_acc_row(i, lane);
                if (co >= c.co) continue;
                if (c.splits > 1) c.partial[(((int64_t)blockIdx.z * c.co + co) * kk2 + tap) * c.ci + ci] = acc[rt][ct][i];
                else c.out[((int64_t)co * c.ci + ci) * kk2 + tap] = acc[rt][ct][i] * c.scale[co];
            }
    }
}

__global__ void __launch_bounds__(256) backbone_wgrad_reduce_kernel(BWgrad c)
{
    const int kk2 = c.ks * c.ks;
    const int64_t total = (int64_t)c.co * kk2 * c.ci, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        float v = c.partial[e];
        for (int z = 1; z < c.splits; ++z) v += c.partial[(int64_t)z * total + e];
        const int ci = (int)(e % c.ci), tap = (int)((e / c.ci) % kk2), co = (int)(e / ((int64_t)c.ci * kk2));
        c.out[((int64_t)co * c.ci + ci) * kk2 + tap] = v * c.scale[co];
    }
}

// ------------------------------------------------------------------------------------------------------------ ingest
// g f32 [B, C, HW] -> out [B, HW, C] compute dtype = (g (+ add)) * (mask > 0)?; 32 pixels x 32 channels per block
template <bool X3>
__global__ void __launch_bounds__(256) backbone_ingest_kernel(const float *g, const char *add, const char *mask, int C, int HW,
                                                              char *out)
{
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32, n = blockIdx.z;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int ch = c0 + ty + 8 * r, p = p0 + tx;
        tile[ty + 8 * r][tx] = ch < C && p < HW ? g[((int64_t)n * C + ch) * HW + p] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int p = p0 + ty + 8 * r, ch = c0 + tx;
        if (p >= HW || ch >= C) continue;
        const int64_t e = ((int64_t)n * HW + p) * C + ch;
        float v = tile[tx][ty + 8 * r];
        if (add) v += load_act<X3>(add, e);
        if (mask && !(load_act<X3>(mask, e) > 0.f)) v = 0.f;
        store_act<X3>(out, e, v);
    }
}

// ------------------------------------------------------------------------------------------------------------ host
int b_out_hw(int in, int k, int s, int p) { return (in + 2 * p - k) / s + 1; }
int b_round32(int v) { return (v + 31) / 32 * 32; }

// the checks every kind shares; fills the output size
// precision and the conv geometry of a dgrad / wgrad op; ho x wo is the size of dz
int check_geometry(const char *what, const sdetr_backbone_bwd_op &o, int precision, int &ho, int &wo)
{
    if (precision != 0 && precision != 1) return fail("%s: precision must be 0 or 1", what);
    if (o.batch < 1 || o.in_channels < 1 || o.out_channels < 1 || o.height < 1 || o.width < 1)
        return fail("%s: bad shape (batch %d, in %d, out %d, %d x %d)", what, o.batch, o.in_channels, o.out_channels,
                    o.height, o.width);
    if ((o.kernel_size != 1 && o.kernel_size != 3) || (o.stride != 1 && o.stride != 2) ||
        o.padding != (o.kernel_size - 1) / 2)
        return fail("%s: unsupported kernel %d / stride %d / padding %d (kernel 1 or 3, stride 1 or 2, padding (k - 1) / 2)",
                    what, o.kernel_size, o.stride, o.padding);
    if (o.in_channels % 32 || o.out_channels % 8)
        return fail("%s: needs in_channels %% 32 == 0 and out_channels %% 8 == 0 (got %d, %d)", what, o.in_channels,
                    o.out_channels);
    ho = b_out_hw(o.height, o.kernel_size, o.stride, o.padding);
    wo = b_out_hw(o.width, o.kernel_size, o.stride, o.padding);
    if (ho < 1 || wo < 1) return fail("%s: empty output", what);
    return 0;
}

int dgrad_splits(int M, int ci, int steps, int stride, int requested)
{
    if (requested > 0) return std::max(1, std::min(requested, std::max(1, steps)));
    const int tiles = ((M / (stride * stride) + kBM - 1) / kBM) * ((ci + kBN - 1) / kBN) * stride * stride;
    if (tiles >= 192) return 1;
    return std::max(1, std::min({8, 256 / tiles, steps / 4}));
}

int make_dgrad(const sdetr_backbone_bwd_op &o, int precision, BDgrad &c)
{
    const char *what = "sdetr_backbone_bwd (dgrad)";
    int ho, wo;
    if (int rc = check_geometry(what, o, precision, ho, wo)) return rc;
    if (!o.dz || !o.weight || !o.out) return fail("%s: null tensor", what);
    if ((reinterpret_cast<uintptr_t>(o.dz) | reinterpret_cast<uintptr_t>(o.weight)) & 15)
        return fail("%s: dz and weight must be 16-byte aligned", what);
    const int64_t esz = precision == 0 ? 4 : 2;
    const int cop = b_round32(o.out_channels), kfull = o.kernel_size * o.kernel_size * cop;
    const int64_t M = (int64_t)o.batch * o.height * o.width;
    const int64_t dz_bytes = (int64_t)o.batch * ho * wo * o.out_channels * esz;
    const int64_t w_bytes = (int64_t)(precision == 0 ? 3 : 1) * o.in_channels * kfull * 2;
    if (M >= (1 << 30) || dz_bytes >= (int64_t(1) << 31) || w_bytes >= (int64_t(1) << 31) ||
        M * o.in_channels >= (int64_t(1) << 31))
        return fail("%s: tensors too large for 32-bit offsets", what);
    c.dz = reinterpret_cast<const char *>(o.dz);
    c.w = reinterpret_cast<const uint16_t *>(o.weight);
    c.add = reinterpret_cast<const char *>(o.add);
    c.mask = reinterpret_cast<const char *>(o.mask);
    c.out = reinterpret_cast<char *>(o.out);
    c.partial = nullptr;
    c.dz_bytes = (uint32_t)dz_bytes;
    c.w_bytes = (uint32_t)w_bytes;
    c.batch = o.batch;
    c.ci = o.in_channels;
    c.h = o.height;
    c.w_in = o.width;
    c.co = o.out_channels;
    c.cop = cop;
    c.ks = o.kernel_size;
    c.stride = o.stride;
    c.pad = o.padding;
    c.ho = ho;
    c.wo = wo;
    c.M = (int)M;
    c.kfull = kfull;
    c.plane = (int64_t)o.in_channels * kfull;
    // the largest class's step count bounds the split (stride 2, 3x3: the odd / odd class has 4 of the 9 taps)
    const int taps = o.stride == 1 ? o.kernel_size * o.kernel_size : (o.kernel_size == 3 ? 4 : 1);
    c.splits = dgrad_splits(c.M, c.ci, taps * (cop / kBK), o.stride, o.splits);
    return 0;
}
int64_t dgrad_workspace(const BDgrad &c) { return c.splits > 1 ? (int64_t)c.splits * c.M * c.ci * 4 : 0; }

int wgrad_splits(int co, int ci, int kk2, int steps, int requested)
{
    if (requested > 0) return std::max(1, std::min(requested, steps));
    const int tiles = ((co + kWM - 1) / kWM) * ((ci + kWN - 1) / kWN) * kk2;
    return std::max(1, std::min({128, (512 + tiles - 1) / tiles, steps / 4}));
}

int make_wgrad(const sdetr_backbone_bwd_op &o, int precision, BWgrad &c)
{
    const char *what = "sdetr_backbone_bwd (wgrad)";
    int ho, wo;
    if (int rc = check_geometry(what, o, precision, ho, wo)) return rc;
    if (!o.dz || !o.x || !o.scale || !o.out) return fail("%s: null tensor", what);
    if ((reinterpret_cast<uintptr_t>(o.dz) | reinterpret_cast<uintptr_t>(o.x)) & 15)
        return fail("%s: dz and x must be 16-byte aligned", what);
    const int64_t esz = precision == 0 ? 4 : 2;
    const int64_t M = (int64_t)o.batch * ho * wo;
    const int64_t dz_bytes = M * o.out_channels * esz;
    const int64_t x_bytes = (int64_t)o.batch * o.height * o.width * o.in_channels * esz;
    if (M >= (1 << 30) || dz_bytes >= (int64_t(1) << 31) || x_bytes >= (int64_t(1) << 31))
        return fail("%s: tensors too large for 32-bit offsets", what);
    c.dz = reinterpret_cast<const char *>(o.dz);
    c.x = reinterpret_cast<const char *>(o.x);
    c.scale = o.scale;
    c.out = reinterpret_cast<float *>(o.out);
    c.partial = nullptr;
    c.dz_bytes = (uint32_t)dz_bytes;
    c.x_bytes = (uint32_t)x_bytes;
    c.batch = o.batch;
    c.ci = o.in_channels;
    c.h = o.height;
    c.w_in = o.width;
    c.co = o.out_channels;
    c.ks = o.kernel_size;
    c.stride = o.stride;
    c.pad = o.padding;
    c.ho = ho;
    c.wo = wo;
    c.M = (int)M;
    const int steps = (c.M + kWK - 1) / kWK;
    c.splits = wgrad_splits(c.co, c.ci, c.ks * c.ks, steps, o.splits);
    c.steps_per_split = (steps + c.splits - 1) / c.splits;
    c.splits = (steps + c.steps_per_split - 1) / c.steps_per_split;
    return 0;
}
int64_t wgrad_workspace(const BWgrad &c)
{
    return c.splits > 1 ? (int64_t)c.splits * c.co * c.ks * c.ks * c.ci * 4 : 0;
}

int check_ingest(const sdetr_backbone_bwd_op &o, int precision)
{
    const char *what = "sdetr_backbone_bwd (ingest)";
    if (precision != 0 && precision != 1) return fail("%s: precision must be 0 or 1", what);
    if (!o.dz || !o.out) return fail("%s: null tensor", what);
    if (o.batch < 1 || o.batch > 65535 || o.in_channels < 1 || o.height < 1 || o.width < 1 ||
        (o.in_channels + 31) / 32 > 65535)
        return fail("%s: bad ingest shape (batch %d, channels %d, %d x %d)", what, o.batch, o.in_channels, o.height, o.width);
    return 0;
}

// validation of one op without a launch; `need` receives its workspace bytes
int check_bwd_op(const sdetr_backbone_bwd_op &o, int precision, int64_t &need)
{
    need = 0;
    if (o.kind == 0) {
        BDgrad c;
        if (int rc = make_dgrad(o, precision, c)) return rc;
        need = dgrad_workspace(c);
        return 0;
    }
    if (o.kind == 1) {
        BWgrad c;
        if (int rc = make_wgrad(o, precision, c)) return rc;
        need = wgrad_workspace(c);
        return 0;
    }
    if (o.kind == 2) return check_ingest(o, precision);
    return fail("sdetr_backbone_bwd: unknown op kind %d", o.kind);
}

template <bool X3>
void launch_dgrad(hipStream_t s, const BDgrad &c)
{
    static DeviceOnce once;
    allow_dynamic_lds(backbone_dgrad_kernel<X3>, once, BCfg<X3>::kLds);
    const int st = c.stride, hc = (c.h + st - 1) / st, wc = (c.w_in + st - 1) / st;   // the largest parity class
    const dim3 grid((unsigned)((c.batch * hc * wc + kBM - 1) / kBM), (unsigned)((c.ci + kBN - 1) / kBN),
                    (unsigned)(st * st * c.splits));
    hipLaunchKernelGGL((backbone_dgrad_kernel<X3>), grid, dim3(kBThreads), BCfg<X3>::kLds, s, c);
    if (c.splits > 1) {
        const unsigned blocks = (unsigned)std::min<int64_t>(((int64_t)c.M * c.ci + 255) / 256, 4096);
        hipLaunchKernelGGL((backbone_dgrad_reduce_kernel<X3>), dim3(blocks), dim3(256), 0, s, c);
    }
}

template <bool X3>
void launch_wgrad(hipStream_t s, const BWgrad &c)
{
    static DeviceOnce once;
    allow_dynamic_lds(backbone_wgrad_kernel<X3>, once, WCfg<X3>::kLds);
    const dim3 grid((unsigned)((c.co + kWM - 1) / kWM), (unsigned)(((c.ci + kWN - 1) / kWN) * c.ks * c.ks), (unsigned)c.splits);
    hipLaunchKernelGGL((backbone_wgrad_kernel<X3>), grid, dim3(kWThreads), WCfg<X3>::kLds, s, c);
    if (c.splits > 1) {
        const unsigned blocks = (unsigned)std::min<int64_t>(((int64_t)c.co * c.ci * c.ks * c.ks + 255) / 256, 4096);
        hipLaunchKernelGGL(backbone_wgrad_reduce_kernel, dim3(blocks), dim3(256), 0, s, c);
    }
}

int run_bwd_op(hipStream_t s, const sdetr_backbone_bwd_op &o, int precision, void *ws, int64_t ws_bytes)
{
    int64_t need;
    if (int rc = check_bwd_op(o, precision, need)) return rc;
    if (need > ws_bytes || (need && !ws))
        return fail("sdetr_backbone_bwd: workspace of %lld bytes is too small (%lld needed)", (long long)ws_bytes,
                    (long long)need);
    if (o.kind == 0) {
        BDgrad c;
        make_dgrad(o, precision, c);
        c.partial = reinterpret_cast<float *>(ws);
        if (precision == 0) launch_dgrad<true>(s, c);
        else launch_dgrad<false>(s, c);
    } else if (o.kind == 1) {
        BWgrad c;
        make_wgrad(o, precision, c);
        c.partial = reinterpret_cast<float *>(ws);
        if (precision == 0) launch_wgrad<true>(s, c);
        else launch_wgrad<false>(s, c);
    } else {
        const int HW = o.height * o.width;
        const dim3 grid((unsigned)((HW + 31) / 32), (unsigned)((o.in_channels + 31) / 32), (unsigned)o.batch);
        if (precision == 0)
            hipLaunchKernelGGL(backbone_ingest_kernel<true>, grid, dim3(256), 0, s, reinterpret_cast<const float *>(o.dz),
                               reinterpret_cast<const char *>(o.add), reinterpret_cast<const char *>(o.mask), o.in_channels,
                               HW, reinterpret_cast<char *>(o.out));
        else
            hipLaunchKernelGGL(backbone_ingest_kernel<false>, grid, dim3(256), 0, s, reinterpret_cast<const float *>(o.dz),
                               reinterpret_cast<const char *>(o.add), reinterpret_cast<const char *>(o.mask), o.in_channels,
                               HW, reinterpret_cast<char *>(o.out));
    }
    return check_launch("sdetr_backbone_bwd");
}

using BackboneBwdPlan = Plan<sdetr_backbone_bwd_op, check_bwd_op, run_bwd_op>;

}  // namespace
}  // namespace sdetr

using namespace sdetr;

extern "C" int64_t sdetr_backbone_dgrad_packed_bytes(int out_channels, int in_channels, int kernel_size, int precision)
{
    if (out_channels < 1 || in_channels < 1 || kernel_size < 1 || (precision != 0 && precision != 1)) return -1;
    return (int64_t)(precision == 0 ? 3 : 1) * in_channels * kernel_size * kernel_size * b_round32(out_channels) * 2;
}

extern "C" int sdetr_backbone_pack_dgrad(sdetr_stream_t stream, const float *weight, const float *gamma,
                                         const float *running_var, float eps, int out_channels, int in_channels,
                                         int kernel_size, int precision, void *packed, float *scale)
{
    if (!weight || !gamma || !running_var || !scale) return fail("sdetr_backbone_pack_dgrad: null tensor");
    if (sdetr_backbone_dgrad_packed_bytes(out_channels, in_channels, kernel_size, precision) < 0)
        return fail("sdetr_backbone_pack_dgrad: bad arguments (out %d, in %d, kernel %d, precision %d)", out_channels,
                    in_channels, kernel_size, precision);
    const int cop = b_round32(out_channels);
    const int64_t total = (int64_t)in_channels * kernel_size * kernel_size * cop;   // (>= out_channels: covers the scale)
    const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(backbone_dgrad_pack_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, weight, gamma,
                       running_var, eps, out_channels, in_channels, kernel_size, cop, precision,
                       reinterpret_cast<uint16_t *>(packed), scale);
    return check_launch("sdetr_backbone_pack_dgrad");
}

extern "C" int sdetr_backbone_bwd_splits(const sdetr_backbone_bwd_op *op, int precision)
{
    if (!op) return fail("sdetr_backbone_bwd_splits: null op");
    if (op->kind == 0) {
        BDgrad c;
        return make_dgrad(*op, precision, c) ? SDETR_EINVAL : c.splits;
    }
    if (op->kind == 1) {
        BWgrad c;
        return make_wgrad(*op, precision, c) ? SDETR_EINVAL : c.splits;
    }
    return fail("sdetr_backbone_bwd_splits: not a dgrad or wgrad op");
}

extern "C" int64_t sdetr_backbone_bwd_workspace_bytes(const sdetr_backbone_bwd_op *ops, int n_ops, int precision)
{
    return BackboneBwdPlan::workspace_bytes(ops, n_ops, precision);
}

extern "C" int sdetr_backbone_dgrad(sdetr_stream_t stream, const sdetr_backbone_bwd_op *op, int precision, void *workspace,
                                    int64_t workspace_bytes)
{
    if (!op || op->kind != 0) return fail("sdetr_backbone_dgrad: not a dgrad op");
    return run_bwd_op((hipStream_t)stream, *op, precision, workspace, workspace_bytes);
}

extern "C" int sdetr_backbone_wgrad(sdetr_stream_t stream, const sdetr_backbone_bwd_op *op, int precision, void *workspace,
                                    int64_t workspace_bytes)
{
    if (!op || op->kind != 1) return fail("sdetr_backbone_wgrad: not a wgrad op");
    return run_bwd_op((hipStream_t)stream, *op, precision, workspace, workspace_bytes);
}

extern "C" int sdetr_backbone_bwd_run(sdetr_stream_t stream, const sdetr_backbone_bwd_op *ops, int n_ops, int precision,
                                      void *workspace, int64_t workspace_bytes)
{
    return BackboneBwdPlan::run("sdetr_backbone_bwd", stream, ops, n_ops, precision, workspace, workspace_bytes);
}

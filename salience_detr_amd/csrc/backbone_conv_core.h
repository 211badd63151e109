// The implicit-GEMM convolution kernel of the backbones, its operand loaders, its epilogues and the host side every family
// shares (fill_conv: a validated geometry as the kernel's arguments; the split of the reduction; the launch).  Used by the
// ResNet (backbone.hip: folded-BN convs, EPI 0), the ConvNeXt (convnext.hip: the two Linears as 1x1 convs and the patchify
// convs, EPI 1 / 2), the FocalNet (focalnet.hip: its Linears, the overlapped patch embedding, and h with the modulation
// product, EPI 3 / 4) and the Swin (swin.hip: its Linears and the stem, EPI 1 / 2 / 5).  What the three row-stream families
// share beyond it (row LayerNorm, host checks): backbone_rows_core.h.  The plan entry points of every family: plan.h.
// Tiles and the MFMA half step: backbone_core.h.
#pragma once

#include <algorithm>
#include <type_traits>

#include "backbone_core.h"
#include "common.h"
#include "gelu_core.h"

namespace sdetr {
namespace {

struct BConv {
    const char *x;          // NHWC compute dtype, or (nchw) the fp32 NCHW canvas
    const uint16_t *w;      // packed [planes][co][kpad]
    const float *bias;      // folded [co]
    const char *res;        // NHWC [M][co] compute dtype, or null
    char *out;              // NHWC [M][co] compute dtype
    float *out_nchw;        // fp32 NCHW [B][co][Ho][Wo], or null
    float *partial;         // split-K pieces [splits][M][co]
    uint32_t x_bytes, w_bytes;
    int batch, ci, h, w_in, co, ks, stride, pad, ho, wo, M, K, kpad, relu, splits, k_per_split;
    int64_t plane;          // co * kpad
    const float *q;         // EPI 3 / 4: the fp32 multiplier rows, element (m, co) at q[m * ldq + co]; EPI 7: q[n]
    int ldq;
    char *aux;              // EPI 6: the pre-GELU values [M][co], compute dtype
    const float *om;        // kADeform: the offset / mask rows [M][32] fp32 (18 offsets, 9 mask logits, 5 unused)
};

// how the A tile is staged: channels-last rows, the stem's NCHW gather, the deformable gather (four masked bilinear
// corners per tap), 16-bit channels-last rows widened to fp32 (the three-way split on 16-bit activations)
constexpr int kANhwc = 0, kANchw = 1, kADeform = 2, kAWiden = 3;

// where output pixel m reads its taps: input row / column of tap (0, 0) and the image's first element
struct RowInfo {
    int iy0, ix0, base;
};
__device__ __forceinline__ RowInfo row_info(const BConv &c, int m, int base_scale)
{
    RowInfo r;
    if (m >= c.M) {
        r.iy0 = -(1 << 28);   // every tap out of range: the row reads zeros
        r.ix0 = 0;
        r.base = 0;
        return r;
    }
    const int hw = c.ho * c.wo, n = m / hw, rem = m - n * hw, oy = rem / c.wo, ox = rem - oy * c.wo;
    r.iy0 = oy * c.stride - c.pad;
    r.ix0 = ox * c.stride - c.pad;
    r.base = n * base_scale;
    return r;
}

// A tile, channels-last input (C % 32 == 0): one tap, 32 contiguous channels per pixel row; 16-byte pieces.
// fp32: 8 pieces per row, rows tid / 8 + 64 j (j < 4); 16-bit: 4 pieces per row, rows tid / 4 + 128 j (j < 2).
template <bool X3>
struct ALoadNHWC {
    static constexpr int kRows = X3 ? 4 : 2, kStep = X3 ? 64 : 128, kShift = X3 ? 3 : 2, kEsz = X3 ? 4 : 2;
    RowInfo ri[kRows];
    uint4 v[kRows];
    __device__ __forceinline__ void init(const BConv &c, int m0, int tid)
    {
#pragma unroll
        for (int j = 0; j < kRows; ++j) ri[j] = row_info(c, m0 + (tid >> kShift) + kStep * j, c.h * c.w_in);
    }
    __device__ __forceinline__ void load(const BConv &c, __amdgpu_buffer_rsrc_t rs, int k0, int kend, int tid)
    {
        const int tap = k0 / c.ci, c0 = k0 - tap * c.ci, ky = tap / c.ks, kx = tap - ky * c.ks;
        const uint32_t piece = 16u * (uint32_t)(tid & ((1 << kShift) - 1));
        const bool kok = k0 < kend;
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const int iy = ri[j].iy0 + ky, ix = ri[j].ix0 + kx;
            const bool ok = kok && (unsigned)iy < (unsigned)c.h && (unsigned)ix < (unsigned)c.w_in;
            const uint32_t pix = (uint32_t)ri[j].base + (uint32_t)iy * (uint32_t)c.w_in + (uint32_t)ix;   // (wraps when !ok)
            v[j] = buffer_load16(rs, b_off(ok, (pix * (uint32_t)c.ci + (uint32_t)c0) * kEsz + piece));
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

// A tile of the exact product on 16-bit activations (the offset / mask conv of a deformable conv in 16-bit mode): the
// 16-bit rows of ALoadNHWC<false>, stored as the fp32 rows the three-way split reads (a 16-bit value splits exactly)
struct ALoadWiden : ALoadNHWC<false> {
    __device__ __forceinline__ void store(char *tile, int tid) const
    {
        char *d = tile + (tid >> 2) * kBRow32 + 32 * (tid & 3);
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const uint4 q = v[j];
            float4 *o = reinterpret_cast<float4 *>(d + kStep * j * kBRow32);
            o[0] = make_float4(act_lo(q.x), act_hi(q.x), act_lo(q.y), act_hi(q.y));
            o[1] = make_float4(act_lo(q.z), act_hi(q.z), act_lo(q.w), act_hi(q.w));
        }
    }
};

// A tile of the modulated deformable 3x3 product: the thread layout of ALoadNHWC, but a tap's 32 channels of a pixel row
// are sum_corner w[corner] * x[corner, c0 .. c0 + 31] with w = bilinear weight * sigmoid(mask logit), zero for a corner
// outside the map and for a sample at y <= -1, y >= H, x <= -1 or x >= W.  The corner rows and weights are computed once
// per tap (a tap spans ci / 32 reduction steps) from the fp32 offset / mask rows c.om.
//
// Addressing: the sample row is by + dy with by the tap's integer row; the coordinate is clamped to [-1, H] in float
// BEFORE the floor and the integer conversion, written on the offset (dy clamped to [-1 - by, H - by], both exact small
// integers) so that floor(by + dy) = by + floor(dy) and the fraction is dy's own: no rounding of the sum, and no offset
// value (huge, infinite, NaN: fmaxf / fminf drop a NaN) reaches the conversion.  Every corner address is clamped into the
// map, an out-of-range corner has weight zero; a row past M reads pixel 0 with weight zero.
template <bool X3>
struct ALoadDeform {
    static constexpr int kRows = X3 ? 4 : 2, kStep = X3 ? 64 : 128, kShift = X3 ? 3 : 2, kEsz = X3 ? 4 : 2;
    int row0, tap_at;
    uint32_t off[kRows][4];   // byte offset of the corner pixel's channel 0: (y0, x0), (y0, x1), (y1, x0), (y1, x1)
    float wt[kRows][4];
    uint4 v[kRows][4];
    __device__ __forceinline__ void init(const BConv &c, int m0, int tid)
    {
        row0 = m0 + (tid >> kShift);
        tap_at = -1;
    }
    __device__ __forceinline__ void corners(const BConv &c, int tap)
    {
        const int ky = tap / 3, kx = tap - 3 * ky;
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            const int m = row0 + kStep * j;
            if (m >= c.M) {
#pragma unroll
                for (int q = 0; q < 4; ++q) off[j][q] = 0u, wt[j][q] = 0.f;
                continue;
            }
            const float *om = c.om + (int64_t)m * 32;
            const RowInfo ri = row_info(c, m, c.h * c.w_in);   // (once per tap: cheaper than nine live registers per row)
            const int by = ri.iy0 + ky, bx = ri.ix0 + kx;
            const float ylo = (float)(-1 - by), yhi = (float)(c.h - by), xlo = (float)(-1 - bx), xhi = (float)(c.w_in - bx);
            const float dy = fminf(fmaxf(om[2 * tap], ylo), yhi), dx = fminf(fmaxf(om[2 * tap + 1], xlo), xhi);
            const bool inside = dy > ylo && dy < yhi && dx > xlo && dx < xhi;
            const float fy = floorf(dy), fx = floorf(dx), ly = dy - fy, lx = dx - fx, hy = 1.f - ly, hx = 1.f - lx;
            const int y0 = by + (int)fy, x0 = bx + (int)fx, y1 = y0 + 1, x1 = x0 + 1;   // in [-1, H] x [-1, W]
            const float mod = inside ? 1.f / (1.f + expf(-om[18 + tap])) : 0.f;
            const bool y0v = y0 >= 0 && y0 < c.h, y1v = y1 >= 0 && y1 < c.h, x0v = x0 >= 0 && x0 < c.w_in, x1v = x1 >= 0 && x1 < c.w_in;
            const uint32_t y0c = (uint32_t)min(max(y0, 0), c.h - 1), y1c = (uint32_t)min(max(y1, 0), c.h - 1);
            const uint32_t x0c = (uint32_t)min(max(x0, 0), c.w_in - 1), x1c = (uint32_t)min(max(x1, 0), c.w_in - 1);
            const uint32_t r0 = (uint32_t)ri.base + y0c * (uint32_t)c.w_in, r1 = (uint32_t)ri.base + y1c * (uint32_t)c.w_in;
            const uint32_t pixel = (uint32_t)c.ci * kEsz;
            off[j][0] = (r0 + x0c) * pixel;
            off[j][1] = (r0 + x1c) * pixel;
            off[j][2] = (r1 + x0c) * pixel;
            off[j][3] = (r1 + x1c) * pixel;
            wt[j][0] = y0v && x0v ? hy * hx * mod : 0.f;
            wt[j][1] = y0v && x1v ? hy * lx * mod : 0.f;
            wt[j][2] = y1v && x0v ? ly * hx * mod : 0.f;
            wt[j][3] = y1v && x1v ? ly * lx * mod : 0.f;
        }
    }
    __device__ __forceinline__ void load(const BConv &c, __amdgpu_buffer_rsrc_t rs, int k0, int kend, int tid)
    {
        if (k0 >= kend) {   // (uniform; K is whole reduction tiles here, so the pipeline never asks)
#pragma unroll
            for (int j = 0; j < kRows; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) v[j][q] = make_uint4(0u, 0u, 0u, 0u);
            return;
        }
        const int tap = k0 / c.ci, c0 = k0 - tap * c.ci;
        if (tap != tap_at) {   // (uniform)
            corners(c, tap);
            tap_at = tap;
        }
        const uint32_t piece = (uint32_t)c0 * kEsz + 16u * (uint32_t)(tid & ((1 << kShift) - 1));
#pragma unroll
        for (int j = 0; j < kRows; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) v[j][q] = buffer_load16(rs, off[j][q] + piece);
    }
    __device__ __forceinline__ void store(char *tile, int tid) const
    {
        constexpr int row = X3 ? kBRow32 : kBRow16;
        char *d = tile + (tid >> kShift) * row + 16 * (tid & ((1 << kShift) - 1));
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
            uint4 r;
            if (X3) {
                float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t u[4] = {v[j][q].x, v[j][q].y, v[j][q].z, v[j][q].w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) s[i] = fmaf(wt[j][q], __uint_as_float(u[i]), s[i]);
                }
                r = make_uint4(__float_as_uint(s[0]), __float_as_uint(s[1]), __float_as_uint(s[2]), __float_as_uint(s[3]));
            } else {   // the four corners summed in fp32, rounded once
                float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const uint32_t u[4] = {v[j][q].x, v[j][q].y, v[j][q].z, v[j][q].w};
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        s[2 * i] = fmaf(wt[j][q], act_lo(u[i]), s[2 * i]);
                        s[2 * i + 1] = fmaf(wt[j][q], act_hi(u[i]), s[2 * i + 1]);
                    }
                }
                r = make_uint4(pack_act2(s[0], s[1]), pack_act2(s[2], s[3]), pack_act2(s[4], s[5]), pack_act2(s[6], s[7]));
            }
            *reinterpret_cast<uint4 *>(d + kStep * j * row) = r;
        }
    }
};

// A tile, the stem: fp32 NCHW canvas, any channel count; 16 reduction indices of one pixel row per thread
template <bool X3>
struct ALoadNCHW {
    RowInfo ri;
    float v[16];
    __device__ __forceinline__ void init(const BConv &c, int m0, int tid)
    {
        ri = row_info(c, m0 + (tid >> 1), c.ci * c.h * c.w_in);
    }
    __device__ __forceinline__ void load(const BConv &c, __amdgpu_buffer_rsrc_t, int k0, int kend, int tid)
    {
        const float *x = reinterpret_cast<const float *>(c.x);
        const int kk2 = c.ks * c.ks, kb = k0 + 16 * (tid & 1), kmax = min(kend, c.K);
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int k = kb + e, ci = k / kk2, t = k - ci * kk2, ky = t / c.ks, kx = t - ky * c.ks;
            const int iy = ri.iy0 + ky, ix = ri.ix0 + kx;
            const bool ok = k < kmax && (unsigned)iy < (unsigned)c.h && (unsigned)ix < (unsigned)c.w_in;
            v[e] = ok ? x[ri.base + ((int64_t)ci * c.h + iy) * c.w_in + ix] : 0.f;
        }
    }
    __device__ __forceinline__ void store(char *tile, int tid) const
    {
        if (X3) {
            char *d = tile + (tid >> 1) * kBRow32 + 64 * (tid & 1);
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *reinterpret_cast<float4 *>(d + 16 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
        } else {
            char *d = tile + (tid >> 1) * kBRow16 + 32 * (tid & 1);
#pragma unroll
            for (int q = 0; q < 2; ++q)
                *reinterpret_cast<uint4 *>(d + 16 * q) =
                    make_uint4(pack_act2(v[8 * q], v[8 * q + 1]), pack_act2(v[8 * q + 2], v[8 * q + 3]),
                               pack_act2(v[8 * q + 4], v[8 * q + 5]), pack_act2(v[8 * q + 6], v[8 * q + 7]));
        }
    }
};

// B tile: the packed weight, 128 output channels x 32 reduction indices per plane, 16 bytes per thread and plane
template <int PL>
struct BLoadW {
    uint4 q[PL];
    __device__ __forceinline__ void load(const BConv &c, __amdgpu_buffer_rsrc_t rs, int n0, int k0, int kend, int tid)
    {
        const int r = n0 + (tid >> 2), k = k0 + 8 * (tid & 3);
        const bool ok = r < c.co && k < kend;
        const uint32_t o = ((uint32_t)r * (uint32_t)c.kpad + (uint32_t)k) * 2u, plane = (uint32_t)(c.plane * 2);
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

// The epilogue of one output element, by EPI:
//   0  relu?(v + b'[co] (+ residual)) -> out (NHWC, compute dtype) and the fp32 NCHW copy (the ResNet's)
//   1  gelu(v + b[co]) -> out (rows, compute dtype): the first Linear of a ConvNeXt block (convnext.hip)
//   2  v + b[co] (+ fp32 residual) -> out (fp32 rows, the ConvNeXt residual stream in every precision) and the NCHW copy
//   3  (v + b[co]) * q[m][co] -> out (rows, compute dtype): FocalNet's h with the modulation product (focalnet.hip)
//   4  the same product -> out (fp32 rows in every precision): h in front of the modulation's own LayerNorm
//   5  v + b[co] -> out (rows, compute dtype): Swin's qkv (swin.hip)
//   6  EPI 1 that also stores v + b[co] -> aux (rows, compute dtype): what a ConvNeXt training forward keeps
//   7  EPI 2 with (v + b[co]) * q[n] before the residual: a ConvNeXt block under stochastic depth (q per sample)
template <bool X3, int EPI>
__device__ __forceinline__ void emit(const BConv &c, int m, int co, float v)
{
    v += c.bias[co];
    const int64_t e = (int64_t)m * c.co + co;
    if (EPI == 1) {
        v = gelu_erf(v);
        if (X3) reinterpret_cast<float *>(c.out)[e] = v;
        else reinterpret_cast<uint16_t *>(c.out)[e] = (uint16_t)f32_to_act_bits(v);
        return;
    }
    if (EPI == 6) {
        if (X3) reinterpret_cast<float *>(c.aux)[e] = v;
        else reinterpret_cast<uint16_t *>(c.aux)[e] = (uint16_t)f32_to_act_bits(v);
        v = gelu_erf(v);
        if (X3) reinterpret_cast<float *>(c.out)[e] = v;
        else reinterpret_cast<uint16_t *>(c.out)[e] = (uint16_t)f32_to_act_bits(v);
        return;
    }
    if (EPI == 5) {
        if (X3) reinterpret_cast<float *>(c.out)[e] = v;
        else reinterpret_cast<uint16_t *>(c.out)[e] = (uint16_t)f32_to_act_bits(v);
        return;
    }
    if (EPI == 3 || EPI == 4) {
        v *= c.q[(int64_t)m * c.ldq + co];
        if (X3 || EPI == 4) reinterpret_cast<float *>(c.out)[e] = v;
        else reinterpret_cast<uint16_t *>(c.out)[e] = (uint16_t)f32_to_act_bits(v);
        return;
    }
    if (EPI == 7) v *= c.q[m / (c.ho * c.wo)];
    if (c.res) {
        if (X3 || EPI == 2 || EPI == 7) v += reinterpret_cast<const float *>(c.res)[e];
        else v += act_lo(reinterpret_cast<const uint16_t *>(c.res)[e]);
    }
    if (EPI == 0 && c.relu) v = fmaxf(v, 0.f);
    if (X3 || EPI == 2 || EPI == 7) reinterpret_cast<float *>(c.out)[e] = v;
    else reinterpret_cast<uint16_t *>(c.out)[e] = (uint16_t)f32_to_act_bits(v);
    if (c.out_nchw) {
        const int hw = c.ho * c.wo, n = m / hw, pix = m - n * hw;
        c.out_nchw[((int64_t)n * c.co + co) * hw + pix] = v;
    }
}

template <bool X3, int AM, int EPI>
__global__ void __launch_bounds__(kBThreads, 1) backbone_conv_kernel(BConv c)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    using Cfg = BCfg<X3>;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * kBM, n0 = blockIdx.y * kBN;
    const int kbeg = blockIdx.z * c.k_per_split, kend = min(c.kpad, kbeg + c.k_per_split);
    const __amdgpu_buffer_rsrc_t rx = make_uniform_rsrc(c.x, c.x_bytes);
    const __amdgpu_buffer_rsrc_t rw = make_uniform_rsrc(reinterpret_cast<const char *>(c.w), c.w_bytes);

    b_f32x16_t acc[2][2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[rt][ct][i] = 0.f;

    static_assert(AM != kAWiden || X3, "widened 16-bit rows feed the three-way split only");
    typename std::conditional<AM == kANchw, ALoadNCHW<X3>,
        typename std::conditional<AM == kADeform, ALoadDeform<X3>,
            typename std::conditional<AM == kAWiden, ALoadWiden, ALoadNHWC<X3>>::type>::type>::type ta;
    BLoadW<X3 ? 3 : 1> tb;
    ta.init(c, m0, tid);
    ta.load(c, rx, kbeg, kend, tid);
    tb.load(c, rw, n0, kbeg, kend, tid);
    ta.store(lds, tid);
    tb.store(lds + Cfg::kA, tid);
    __syncthreads();
    const int fa = X3 ? (64 * wm + (lane & 31)) * kBRow32 + (lane >> 5) * 32 : (64 * wm + (lane & 31)) * kBRow16 + (lane >> 5) * 16;
    const int fb = Cfg::kA + (64 * wn + (lane & 31)) * kBRow16 + (lane >> 5) * 16;
    int cur = 0;
    for (int k0 = kbeg; k0 < kend; k0 += kBK) {
        const bool more = k0 + kBK < kend;   // (uniform)
        if (more) {                          // the next tile travels in registers while this one is multiplied
            ta.load(c, rx, k0 + kBK, kend, tid);
            tb.load(c, rw, n0, k0 + kBK, kend, tid);
        }
        const char *s = lds + cur * Cfg::kStage;
        half_step<X3>(s + fa, s + fb, 0, acc);
        half_step<X3>(s + fa, s + fb, 1, acc);
        if (more) {   // the other stage's last readers passed the previous barrier
            char *d = lds + (cur ^ 1) * Cfg::kStage;
            ta.store(d, tid);
            tb.store(d + Cfg::kA, tid);
        }
        __syncthreads();
        cur ^= 1;
    }

#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int co = n0 + 64 * wn + 32 * ct + (lane & 31);
        if (co >= c.co) continue;
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int m = m0 + 64 * wm + 32 * rt + b_acc_row(i, lane);
                if (m >= c.M) continue;
                if (c.splits > 1) c.partial[((int64_t)blockIdx.z * c.M + m) * c.co + co] = acc[rt][ct][i];
                else emit<X3, EPI>(c, m, co, acc[rt][ct][i]);
            }
    }
}

// the split-K pieces summed in split order (deterministic), then the epilogue
template <bool X3, int EPI>
__global__ void __launch_bounds__(256) backbone_splitk_kernel(BConv c)
{
    const int64_t total = (int64_t)c.M * c.co, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        float v = c.partial[e];
        for (int z = 1; z < c.splits; ++z) v += c.partial[(int64_t)z * total + e];
        const int m = (int)(e / c.co), co = (int)(e - (int64_t)m * c.co);
        emit<X3, EPI>(c, m, co, v);
    }
}

// ---- host: the split of the reduction and the launch (the conv kernel, then the fixed-order sum of its pieces)
int out_hw(int in, int k, int s, int p) { return (in + 2 * p - k) / s + 1; }
int round32(int v) { return (v + 31) / 32 * 32; }

int resolve_splits(int M, int co, int kpad, int requested)
{
    const int steps = kpad / kBK;
    if (requested > 0) return std::max(1, std::min(requested, steps));
    const int tiles = ((M + kBM - 1) / kBM) * ((co + kBN - 1) / kBN);
    if (tiles >= 192) return 1;
    return std::max(1, std::min({8, 256 / tiles, steps / 4}));
}

// The geometry of one conv op, already checked against its family's rules: the tensors, the input [batch, h, w, ci] (or with
// x_nchw the fp32 NCHW canvas), the kernel, and the op's own output size.
struct ConvGeom {
    const void *x, *weight;
    const float *bias;
    const void *residual;
    void *out;
    int batch, ci, h, w, co, ks, stride, pad, ho, wo, x_nchw, splits;
};

// c = the kernel's arguments for g: every member set (those a family adds afterwards -- out_nchw, q / ldq, aux, relu -- start
// null / 0), K padded to whole reduction tiles, the 32-bit size limits, the resolved split of the reduction
int fill_conv(const char *what, const ConvGeom &g, int precision, BConv &c)
{
    c = BConv{};
    c.x = reinterpret_cast<const char *>(g.x);
    c.w = reinterpret_cast<const uint16_t *>(g.weight);
    c.bias = g.bias;
    c.res = reinterpret_cast<const char *>(g.residual);
    c.out = reinterpret_cast<char *>(g.out);
    c.batch = g.batch;
    c.ci = g.ci;
    c.h = g.h;
    c.w_in = g.w;
    c.co = g.co;
    c.ks = g.ks;
    c.stride = g.stride;
    c.pad = g.pad;
    c.ho = g.ho;
    c.wo = g.wo;
    c.K = g.ci * g.ks * g.ks;
    c.kpad = round32(c.K);
    const int64_t M = (int64_t)g.batch * g.ho * g.wo;
    const int64_t esz = (g.x_nchw || precision == 0) ? 4 : 2;
    const int64_t x_bytes = (int64_t)g.batch * g.ci * g.h * g.w * esz;
    const int64_t w_bytes = (int64_t)(precision == 0 ? 3 : 1) * g.co * c.kpad * 2;
    if (M >= (1 << 30) || x_bytes >= (int64_t(1) << 31) || w_bytes >= (int64_t(1) << 31) || M * g.co >= (int64_t(1) << 31))
        return fail("%s: tensors too large for 32-bit offsets", what);
    c.M = (int)M;
    c.x_bytes = (uint32_t)x_bytes;
    c.w_bytes = (uint32_t)w_bytes;
    c.plane = (int64_t)g.co * c.kpad;
    c.splits = resolve_splits(c.M, c.co, c.kpad, g.splits);
    c.k_per_split = (c.kpad / kBK + c.splits - 1) / c.splits * kBK;
    c.splits = (c.kpad + c.k_per_split - 1) / c.k_per_split;
    return 0;
}

int64_t conv_workspace(const BConv &c) { return c.splits > 1 ? (int64_t)c.splits * c.M * c.co * 4 : 0; }

template <bool X3, int AM, int EPI>
void launch_conv(hipStream_t s, const BConv &c)
{
    static DeviceOnce once;
    allow_dynamic_lds(backbone_conv_kernel<X3, AM, EPI>, once, BCfg<X3>::kLds);
    const dim3 grid((unsigned)((c.M + kBM - 1) / kBM), (unsigned)((c.co + kBN - 1) / kBN), (unsigned)c.splits);
    hipLaunchKernelGGL((backbone_conv_kernel<X3, AM, EPI>), grid, dim3(kBThreads), BCfg<X3>::kLds, s, c);
    if (c.splits > 1) {
        const int64_t total = (int64_t)c.M * c.co;
        const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 4096);
        hipLaunchKernelGGL((backbone_splitk_kernel<X3, EPI>), dim3(blocks), dim3(256), 0, s, c);
    }
}

}  // namespace
}  // namespace sdetr

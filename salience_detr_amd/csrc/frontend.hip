// The detector's input stage (row N7): ChannelMapper convolutions + GroupNorm, per-level padding masks and sine positions
// (reference models/necks/channel_mapper.py, models/bricks/position_encoding.py:9-67, salience_detr.py:172-176).
//
//   frontend_conv_kernel        every 1x1 level and the 3x3 stride-2 extra level in ONE launch, C[co, p] = W[co, k] X[k, p]
//                               per image on the matrix cores; the 1x1 epilogue writes NCHW and per-(image, channel,
//                               pixel tile) GroupNorm partials (mean, M2); the 3x3 level is split over K into partial sums
//   frontend_groupnorm_kernel   every level in one launch: merges the partials in a fixed order (Chan's formula, no
//                               atomics), reduces the 3x3 split-K sums, applies (x - mean) * rstd * gamma + beta in place;
//                               <true> is the training forward's (sdetr_frontend_groupnorm_train): it also keeps the raw
//                               convolution and the statistics for frontend_backward.hip
//   frontend_positions_kernel   all levels' nearest-down-sampled masks and sine position maps in one launch
//
// GEMM tiles: 128 output channels x 128 pixels x 32 reduction indices, 4 waves of 64 x 64 (2 x 2 v_mfma_f32_32x32x16 per
// 16-deep step), operands staged in LDS as fp32 rows [row][k] (row stride 144 bytes), the structure of gemm_x3.hip's
// first-generation kernel.  A = the weight [Co][K] (k-major); B = the backbone map as it lies: the reduction index (input
// channel) is the row, pixels contiguous -- the loader transposes 4 x 4 blocks in registers.  The 3x3 form gathers
// its B tile (implicit GEMM, k = ci * 9 + ky * 3 + kx, the weight's own layout).  fp32 precision: both operands are split
// exactly into three bf16 terms and six products are accumulated (gemm_x3.hip) -- the weight once, when it is packed
// (frontend_pack_kernel, three planes), the map fragment by fragment; 16-bit precision: one product of the
// round-to-nearest 16-bit operands (bf16 here, fp16 in libsalience_hip_f16.so; the weight packed as one plane), fp32
// accumulation and output.
#include <algorithm>

#include "common.h"

namespace sdetr {
namespace {

constexpr int kFTile = 128, kFK = 32, kFThreads = 256;
constexpr int kFRow = kFK * 4 + 16;                 // bytes per fp32 operand row in LDS
constexpr int kFBOperand = kFTile * kFRow;          // 18 432: the fp32 B tile
constexpr int kFPreRow = kFK * 2 + 16;              // bytes per row of a packed 16-bit weight plane in LDS
constexpr int kFPrePlane = kFTile * kFPreRow;       // 10 240
constexpr int kFAOperand = 3 * kFPrePlane;          // 30 720: up to three planes of the A tile
constexpr int kFCStride = kFTile + 4;               // floats per row of the staged C tile
constexpr int kFLds = kFTile * kFCStride * 4;       // 67 584 (the staged C tile)
static_assert(kFAOperand + kFBOperand <= kFLds, "operand tiles fit in the C tile's LDS");
constexpr int kFMaxLevels = 8;
constexpr int kFNormChunk = 4096;                   // elements per groupnorm workgroup (1x1 levels)

typedef __bf16 f_bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f_f32x16_t __attribute__((ext_vector_type(16)));

struct ConvLevel {
    const float *x;          // [B, Cin, H, W]
    const uint16_t *w;       // packed weight [planes][Co][K] (sdetr_frontend_pack_weight)
    float *out;              // 1x1: [B, Co, H, W] (raw conv, normalised later in place); 3x3: split partials [S][B][Co][P]
    float *stats;            // 1x1: [B][Co][tiles_n][2] (mean, M2)
    int cin, h, w_in, ho, wo, kernel, K, P, tiles_n, tiles_m, splits, k_per_split;
    int block0;              // first block of this level in the launch
    int64_t plane;           // elements between the weight's planes (Co * K)
};
struct ConvArgs {
    ConvLevel lv[kFMaxLevels];
    int n_levels, batch, co, precision;
};

__device__ __forceinline__ int f_acc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

__device__ __forceinline__ uint32_t f_pack_hi(float lo, float hi)
{
    return __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo), 0x07060302u);
}

// exact three-way bf16 split of 8 fp32 values (truncation: h = top 16 bits, r1 = x - h, m = top 16 bits of r1, r2 = r1 - m)
struct FFrag3 {
    u32x4_t p[3];
};
__device__ __forceinline__ FFrag3 f_split(const float4 lo, const float4 hi)
{
    const float x[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    float r1[8], r2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        r1[i] = x[i] - __uint_as_float(__float_as_uint(x[i]) & 0xffff0000u);
        r2[i] = r1[i] - __uint_as_float(__float_as_uint(r1[i]) & 0xffff0000u);
    }
    FFrag3 f;
    f.p[0] = u32x4_t{f_pack_hi(x[0], x[1]), f_pack_hi(x[2], x[3]), f_pack_hi(x[4], x[5]), f_pack_hi(x[6], x[7])};
    f.p[1] = u32x4_t{f_pack_hi(r1[0], r1[1]), f_pack_hi(r1[2], r1[3]), f_pack_hi(r1[4], r1[5]), f_pack_hi(r1[6], r1[7])};
    f.p[2] = u32x4_t{f_pack_hi(r2[0], r2[1]), f_pack_hi(r2[2], r2[3]), f_pack_hi(r2[4], r2[5]), f_pack_hi(r2[6], r2[7])};
    return f;
}
__device__ __forceinline__ uint4 f_round16(const float4 lo, const float4 hi)
{
    return make_uint4(pack_act2(lo.x, lo.y), pack_act2(lo.z, lo.w), pack_act2(hi.x, hi.y), pack_act2(hi.z, hi.w));
}
__device__ __forceinline__ f_f32x16_t f_mfma_bf16(u32x4_t a, u32x4_t b, f_f32x16_t c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(f_bf16x8_t, a), __builtin_bit_cast(f_bf16x8_t, b), c, 0,
                                                   0, 0);
}

// A tile: PL planes of the packed weight, rows m0.. (k-major, K a multiple of 32); each thread 16 elements of one row
// per plane.  LDS: [plane][row][k] 16-bit, rows 80 bytes apart (conflict-free 16-byte fragment reads, as gemm_x3.hip's
// pre-split operand).
template <int PL>
struct ALoad {
    uint4 q[PL][2];
    __device__ __forceinline__ void load(const uint16_t *w, int K, int64_t plane, int rows, int m0, int k0, int kend, int tid)
    {
        const int r = m0 + (tid >> 1), k = k0 + 16 * (tid & 1);
        const uint16_t *src = w + (int64_t)r * K + k;
        const bool ok = r < rows && k < kend;   // (k .. k + 15 all inside: K and the split bounds are multiples of 32)
#pragma unroll
        for (int pl = 0; pl < PL; ++pl) {
            q[pl][0] = ok ? *reinterpret_cast<const uint4 *>(src + pl * plane) : make_uint4(0u, 0u, 0u, 0u);
            q[pl][1] = ok ? *reinterpret_cast<const uint4 *>(src + pl * plane + 8) : make_uint4(0u, 0u, 0u, 0u);
        }
    }
    __device__ __forceinline__ void store(char *planes, int tid) const
    {
        char *d = planes + (tid >> 1) * kFPreRow + 32 * (tid & 1);
#pragma unroll
        for (int pl = 0; pl < PL; ++pl) {
            *reinterpret_cast<uint4 *>(d + pl * kFPrePlane) = q[pl][0];
            *reinterpret_cast<uint4 *>(d + pl * kFPrePlane + 16) = q[pl][1];
        }
    }
};

// B tile: 4 pixels x 4 reduction indices per thread (v_j = the 4 pixels at reduction index k + j), stored transposed
// as [pixel][k].  Out-of-range pixels, reduction indices and (3x3) padding taps read as zero.
struct BLoad {
    float4 v0, v1, v2, v3;   // (named members: an array here ends up in scratch memory)
    __device__ __forceinline__ static float4 row4(const ConvLevel &L, const float *x, int p, int k, int kend, bool vec)
    {
        const float *q = x + (int64_t)k * L.P + p;
        const bool kok = k < kend;
        if (vec) return kok ? *reinterpret_cast<const float4 *>(q) : make_float4(0.f, 0.f, 0.f, 0.f);
        return make_float4(kok && p < L.P ? q[0] : 0.f, kok && p + 1 < L.P ? q[1] : 0.f, kok && p + 2 < L.P ? q[2] : 0.f,
                           kok && p + 3 < L.P ? q[3] : 0.f);
    }
    // 3x3 stride-2 pad-1 tap of output pixel pi at reduction index kk = ci * 9 + ky * 3 + kx
    __device__ __forceinline__ static float tap(const ConvLevel &L, const float *x, int pi, int kk, int kend)
    {
        const int oy = pi / L.wo, ox = pi - oy * L.wo;
        const int ci = kk / 9, t = kk - ci * 9;
        const int iy = 2 * oy - 1 + t / 3, ix = 2 * ox - 1 + t % 3;
        const bool ok = pi < L.P && kk < kend && iy >= 0 && iy < L.h && ix >= 0 && ix < L.w_in;
        return ok ? x[((int64_t)ci * L.h + iy) * L.w_in + ix] : 0.f;
    }
    __device__ __forceinline__ static float4 taps4(const ConvLevel &L, const float *x, int p, int kk, int kend)
    {
        return make_float4(tap(L, x, p, kk, kend), tap(L, x, p + 1, kk, kend), tap(L, x, p + 2, kk, kend),
                           tap(L, x, p + 3, kk, kend));
    }
    __device__ __forceinline__ void load(const ConvLevel &L, const float *x, int n0, int k0, int kend, int tid)
    {
        const int kb = tid & 7, mb = tid >> 3;
        const int p = n0 + 4 * mb, k = k0 + 4 * kb;
        if (L.kernel == 1) {
            const bool vec = (L.P & 3) == 0 && p + 3 < L.P;
            v0 = row4(L, x, p, k, kend, vec);
            v1 = row4(L, x, p, k + 1, kend, vec);
            v2 = row4(L, x, p, k + 2, kend, vec);
            v3 = row4(L, x, p, k + 3, kend, vec);
        } else {
            v0 = taps4(L, x, p, k, kend);
            v1 = taps4(L, x, p, k + 1, kend);
            v2 = taps4(L, x, p, k + 2, kend);
            v3 = taps4(L, x, p, k + 3, kend);
        }
    }
    __device__ __forceinline__ void store(char *tile, int tid) const
    {
        const int kb = tid & 7, mb = tid >> 3;
        char *d = tile + (4 * mb) * kFRow + 16 * kb;
        *reinterpret_cast<float4 *>(d) = make_float4(v0.x, v1.x, v2.x, v3.x);
        *reinterpret_cast<float4 *>(d + kFRow) = make_float4(v0.y, v1.y, v2.y, v3.y);
        *reinterpret_cast<float4 *>(d + 2 * kFRow) = make_float4(v0.z, v1.z, v2.z, v3.z);
        *reinterpret_cast<float4 *>(d + 3 * kFRow) = make_float4(v0.w, v1.w, v2.w, v3.w);
    }
};

template <bool X3>
__device__ __forceinline__ void conv_step(const ConvLevel &L, const float *x, ALoad<X3 ? 3 : 1> &ta, BLoad &tb, char *pa,
                                          char *pb,
                                          const char *fa, const char *fb, int m0, int n0, int rows, int k0, int kend,
                                          int tid, f_f32x16_t (&acc)[2][2])
{
    ta.store(pa, tid);
    tb.store(pb, tid);
    __syncthreads();
    ta.load(L.w, L.K, L.plane, rows, m0, k0 + 2 * kFK, kend, tid);   // two steps ahead (zeros past the end)
    tb.load(L, x, n0, k0 + 2 * kFK, kend, tid);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        const char *a0 = fa + kk * 32, *a1 = fa + 32 * kFPreRow + kk * 32;
        const float4 *qb0 = reinterpret_cast<const float4 *>(fb + kk * 64);
        const float4 *qb1 = reinterpret_cast<const float4 *>(fb + 32 * kFRow + kk * 64);
        if (X3) {
            FFrag3 fa3[2];   // the weight's three bf16 terms, split once when it was packed
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                fa3[0].p[pl] = *reinterpret_cast<const u32x4_t *>(a0 + pl * kFPrePlane);
                fa3[1].p[pl] = *reinterpret_cast<const u32x4_t *>(a1 + pl * kFPrePlane);
            }
            const FFrag3 fb3[2] = {f_split(qb0[0], qb0[1]), f_split(qb1[0], qb1[1])};
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    f_f32x16_t c = acc[rt][ct];
                    c = f_mfma_bf16(fa3[rt].p[2], fb3[ct].p[0], c);   // smallest terms first
                    c = f_mfma_bf16(fa3[rt].p[0], fb3[ct].p[2], c);
                    c = f_mfma_bf16(fa3[rt].p[1], fb3[ct].p[1], c);
                    c = f_mfma_bf16(fa3[rt].p[1], fb3[ct].p[0], c);
                    c = f_mfma_bf16(fa3[rt].p[0], fb3[ct].p[1], c);
                    c = f_mfma_bf16(fa3[rt].p[0], fb3[ct].p[0], c);
                    acc[rt][ct] = c;
                }
        } else {
            const uint4 a16[2] = {*reinterpret_cast<const uint4 *>(a0), *reinterpret_cast<const uint4 *>(a1)};
            const uint4 b16[2] = {f_round16(qb0[0], qb0[1]), f_round16(qb1[0], qb1[1])};
#pragma unroll
            for (int rt = 0; rt < 2; ++rt)
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) acc[rt][ct] = mfma_act_32x32x16(a16[rt], b16[ct], acc[rt][ct]);
        }
    }
    __syncthreads();
}

// (mean, M2, count) of two disjoint sets -> their union (Chan et al.); count 0 on either side is exact
__device__ __forceinline__ void chan_merge(float &mean, float &m2, float &n, float mb, float m2b, float nb)
{
    const float t = n + nb;
    if (nb == 0.f) return;
    const float d = mb - mean, f = nb / t;
    mean += d * f;
    m2 += m2b + d * d * n * f;
    n = t;
}

template <bool X3>
__global__ void __launch_bounds__(kFThreads, 2) frontend_conv_kernel(ConvArgs p)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    int li = 0;
    for (int i = 1; i < p.n_levels; ++i)
        if ((int)blockIdx.x >= p.lv[i].block0) li = i;
    const ConvLevel &L = p.lv[li];
    int r = blockIdx.x - L.block0;
    const int tn = r % L.tiles_n; r /= L.tiles_n;
    const int tm = r % L.tiles_m; r /= L.tiles_m;
    const int img = r % p.batch;
    const int split = r / p.batch;

    char *pa = lds, *pb = lds + kFAOperand;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = tm * kFTile, n0 = tn * kFTile;
    const int kbeg = split * L.k_per_split, kend = min(L.K, kbeg + L.k_per_split);
    const float *x = L.x + (int64_t)img * L.cin * L.h * L.w_in;

    f_f32x16_t acc[2][2];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[rt][ct][i] = 0.f;

    ALoad<X3 ? 3 : 1> ta0, ta1;
    BLoad tb0, tb1;
    ta0.load(L.w, L.K, L.plane, p.co, m0, kbeg, kend, tid);
    tb0.load(L, x, n0, kbeg, kend, tid);
    ta1.load(L.w, L.K, L.plane, p.co, m0, kbeg + kFK, kend, tid);
    tb1.load(L, x, n0, kbeg + kFK, kend, tid);
    const char *fa = pa + (64 * wm + (lane & 31)) * kFPreRow + (lane >> 5) * 16;
    const char *fb = pb + (64 * wn + (lane & 31)) * kFRow + (lane >> 5) * 32;
    for (int k0 = kbeg; k0 < kend; k0 += 2 * kFK) {
        conv_step<X3>(L, x, ta0, tb0, pa, pb, fa, fb, m0, n0, p.co, k0, kend, tid, acc);
        if (k0 + kFK < kend) conv_step<X3>(L, x, ta1, tb1, pa, pb, fa, fb, m0, n0, p.co, k0 + kFK, kend, tid, acc);
    }

    // stage the C tile in LDS (the operand tiles are no longer read: the last step ended on a barrier)
    float *ct_lds = reinterpret_cast<float *>(lds);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int m = 64 * wm + 32 * rt + f_acc_row(i, lane), n = 64 * wn + 32 * ct + (lane & 31);
                ct_lds[m * kFCStride + n] = acc[rt][ct][i];
            }
    __syncthreads();

    const int rows = min(kFTile, p.co - m0), cols = min(kFTile, L.P - n0);
    float *dst = L.kernel == 1 ? L.out + ((int64_t)img * p.co + m0) * L.P + n0
                               : L.out + (((int64_t)split * p.batch + img) * p.co + m0) * L.P + n0;
    for (int e = tid; e < kFTile * kFTile; e += kFThreads) {   // rows of 128 consecutive pixels: coalesced NCHW
        const int m = e >> 7, n = e & 127;
        if (m < rows && n < cols) dst[(int64_t)m * L.P + n] = ct_lds[m * kFCStride + n];
    }
    if (L.kernel != 1) return;
    // GroupNorm partials of this tile: per output channel, (mean, M2) over its `cols` pixels; two threads per channel
    // (64 pixels each, exact two-pass), merged by Chan's formula -- fixed order, no atomics
    const int m = tid >> 1, half = tid & 1;
    const int c0 = 64 * half, cnt = max(0, min(64, cols - c0));
    const float *row = ct_lds + m * kFCStride + c0;
    float s = 0.f;
    for (int n = 0; n < cnt; ++n) s += row[n];
    float mean = cnt ? s / (float)cnt : 0.f, m2 = 0.f;
    for (int n = 0; n < cnt; ++n) {
        const float d = row[n] - mean;
        m2 += d * d;
    }
    float nn = (float)cnt;
    const float mean_b = __shfl_xor(mean, 1), m2_b = __shfl_xor(m2, 1), n_b = __shfl_xor(nn, 1);
    if (half == 0 && m < rows) {
        chan_merge(mean, m2, nn, mean_b, m2_b, n_b);
        float *st = L.stats + (((int64_t)img * p.co + m0 + m) * L.tiles_n + tn) * 2;
        st[0] = mean;
        st[1] = m2;
    }
}

// ---- GroupNorm finalize + apply ------------------------------------------------------------------------------------
struct NormLevel {
    float *out;              // [B, Co, P], normalised in place (3x3: written here from the partials)
    const float *part;       // 1x1: stats [B][Co][tiles_n][2]; 3x3: split sums [S][B][Co][P]
    const float *gamma, *beta;
    float *z;                // training forward: the raw convolution [B, Co, P] (a buffer of its own)
    float *stats;            // training forward: [B][groups][2] = (mean, rstd)
    int P, kernel, tiles_n, splits, chunks;
    int block0;
};
struct NormArgs {
    NormLevel lv[kFMaxLevels];
    int n_levels, batch, co, groups;
    float eps;
};

// merge (mean, M2, n) across the workgroup in a fixed tree order
__device__ __forceinline__ void block_merge(float &mean, float &m2, float &n, float *red)
{
    const int tid = threadIdx.x;
    red[tid] = mean; red[kFThreads + tid] = m2; red[2 * kFThreads + tid] = n;
    __syncthreads();
    for (int w = kFThreads / 2; w > 0; w >>= 1) {
        if (tid < w) {
            float a = red[tid], b = red[kFThreads + tid], c = red[2 * kFThreads + tid];
            chan_merge(a, b, c, red[tid + w], red[kFThreads + tid + w], red[2 * kFThreads + tid + w]);
            red[tid] = a; red[kFThreads + tid] = b; red[2 * kFThreads + tid] = c;
        }
        __syncthreads();
    }
    mean = red[0]; m2 = red[kFThreads]; n = red[2 * kFThreads];
}

// TRAIN: the same arithmetic in the same order (the output is bit-identical), and what the backward reads on the side:
// the raw convolution to L.z and the group's (mean, rstd) to L.stats
template <bool TRAIN>
__global__ void __launch_bounds__(kFThreads) frontend_groupnorm_kernel(NormArgs p)
{
    __shared__ float red[3 * kFThreads];
    int li = 0;
    for (int i = 1; i < p.n_levels; ++i)
        if ((int)blockIdx.x >= p.lv[i].block0) li = i;
    const NormLevel &L = p.lv[li];
    int r = blockIdx.x - L.block0;
    const int chunk = r % L.chunks; r /= L.chunks;
    const int g = r % p.groups;
    const int img = r / p.groups;
    const int cg = p.co / p.groups, tid = threadIdx.x;
    const int64_t glen = (int64_t)cg * L.P;
    float *y = L.out + ((int64_t)img * p.co + (int64_t)g * cg) * L.P;   // the group's channels are contiguous
    float *zs = TRAIN ? L.z + ((int64_t)img * p.co + (int64_t)g * cg) * L.P : nullptr;
    float mean = 0.f, m2 = 0.f, n = 0.f;
    if (L.kernel == 1) {
        const int items = cg * L.tiles_n;
        for (int i = tid; i < items; i += kFThreads) {
            const int c = i / L.tiles_n, t = i - c * L.tiles_n;
            const float *st = L.part + (((int64_t)img * p.co + g * cg + c) * L.tiles_n + t) * 2;
            chan_merge(mean, m2, n, st[0], st[1], (float)min(kFTile, L.P - t * kFTile));
        }
    } else {
        // reduce the split-K partial sums (fixed split order) into the output, Welford per thread
        const int64_t split_stride = (int64_t)p.batch * p.co * L.P;
        const float *src = L.part + ((int64_t)img * p.co + (int64_t)g * cg) * L.P;
        for (int64_t e = tid; e < glen; e += kFThreads) {
            float v = 0.f;
            for (int s = 0; s < L.splits; ++s) v += src[s * split_stride + e];
            y[e] = v;
            if (TRAIN) zs[e] = v;
            n += 1.f;
            const float d = v - mean;
            mean += d / n;
            m2 += d * (v - mean);
        }
    }
    block_merge(mean, m2, n, red);
    const float rstd = 1.f / sqrtf(fmaxf(m2 / n, 0.f) + p.eps);
    int64_t e0 = 0, e1 = glen;
    if (L.kernel == 1) {
        e0 = (int64_t)chunk * kFNormChunk;
        e1 = min(glen, e0 + kFNormChunk);
    }
    // (3x3: each thread re-reads exactly the elements it wrote above)
    if (TRAIN && chunk == 0 && tid == 0) {
        float *st = L.stats + ((int64_t)img * p.groups + g) * 2;
        st[0] = mean;
        st[1] = rstd;
    }
    for (int64_t e = e0 + tid; e < e1; e += kFThreads) {
        const int c = g * cg + (int)(e / L.P);
        const float v = y[e];
        if (TRAIN && L.kernel == 1) zs[e] = v;
        y[e] = (v - mean) * rstd * L.gamma[c] + L.beta[c];
    }
}

// ---- masks + sine positions ----------------------------------------------------------------------------------------
struct PosLevel {
    uint8_t *mask;           // [B, Hl, Wl] bool
    float *pos;              // [B, 2F, Hl, Wl]
    int h, w, block0;
};
struct PosArgs {
    PosLevel lv[kFMaxLevels];
    const uint8_t *src;      // [B, H, W] bool, True on padding
    const float *dim_ty, *dim_tx;   // [F]
    int n_levels, batch, H, W, F, normalize;
    float scale, eps, offset;
};

__global__ void __launch_bounds__(kFThreads) frontend_positions_kernel(PosArgs p)
{
    int li = 0;
    for (int i = 1; i < p.n_levels; ++i)
        if ((int)blockIdx.x >= p.lv[i].block0) li = i;
    const PosLevel &L = p.lv[li];
    const int64_t e = (int64_t)(blockIdx.x - L.block0) * kFThreads + threadIdx.x;
    const int64_t hw = (int64_t)L.h * L.w;
    if (e >= (int64_t)p.batch * hw) return;
    const int b = (int)(e / hw);
    const int yx = (int)(e - (int64_t)b * hw);
    const int y = yx / L.w, x = yx - y * L.w;
    // torch's "nearest" source pixel: min(int(floorf(dst * (float)in / out)), in - 1)
    const float sh = (float)p.H / (float)L.h, sw = (float)p.W / (float)L.w;
    const uint8_t *src = p.src + (int64_t)b * p.H * p.W;
    const int sx = min((int)floorf((float)x * sw), p.W - 1), sy = min((int)floorf((float)y * sh), p.H - 1);
    float cy = 0.f, ty = 0.f, cx = 0.f, tx = 0.f;   // valid counts (exact integers in fp32)
    for (int yy = 0; yy < L.h; ++yy) {
        const int syy = min((int)floorf((float)yy * sh), p.H - 1);
        const float v = src[(int64_t)syy * p.W + sx] ? 0.f : 1.f;
        ty += v;
        if (yy <= y) cy += v;
    }
    for (int xx = 0; xx < L.w; ++xx) {
        const int sxx = min((int)floorf((float)xx * sw), p.W - 1);
        const float v = src[(int64_t)sy * p.W + sxx] ? 0.f : 1.f;
        tx += v;
        if (xx <= x) cx += v;
    }
    L.mask[e] = src[(int64_t)sy * p.W + sx] ? 1 : 0;
    float ey, ex;
    if (p.normalize) {   // the reference's fp32 order: (cumsum + offset) / (last + eps) * scale
        ey = (cy + p.offset) / (ty + p.eps) * p.scale;
        ex = (cx + p.offset) / (tx + p.eps) * p.scale;
    } else {
        ey = cy + p.offset;
        ex = cx + p.offset;
    }
    float *out = L.pos + (int64_t)b * 2 * p.F * hw + yx;
    for (int c = 0; c < p.F; ++c) {
        const float a = ey / p.dim_ty[c];   // a true division, as the reference's
        out[(int64_t)c * hw] = (c & 1) ? cosf(a) : sinf(a);
    }
    for (int c = 0; c < p.F; ++c) {
        const float a = ex / p.dim_tx[c];
        out[(int64_t)(p.F + c) * hw] = (c & 1) ? cosf(a) : sinf(a);
    }
}

// the packed weight: precision 0 -> three planes [3][n] of the exact truncating bf16 split (the terms f_split makes);
// precision 1 -> one plane [n] rounded to nearest (this library's 16-bit type)
__global__ void __launch_bounds__(kFThreads) frontend_pack_kernel(const float *w, int64_t n, int precision, uint16_t *out)
{
    for (int64_t i = (int64_t)blockIdx.x * kFThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kFThreads) {
        const float x = w[i];
        if (precision == 0) {
            const float r1 = x - __uint_as_float(__float_as_uint(x) & 0xffff0000u);
            const float r2 = r1 - __uint_as_float(__float_as_uint(r1) & 0xffff0000u);
            out[i] = (uint16_t)(__float_as_uint(x) >> 16);
            out[n + i] = (uint16_t)(__float_as_uint(r1) >> 16);
            out[2 * n + i] = (uint16_t)(__float_as_uint(r2) >> 16);
        } else {
            out[i] = (uint16_t)(pack_act2(x, 0.f) & 0xffffu);
        }
    }
}

DeviceOnce g_conv_lds_x3, g_conv_lds_16;

struct Plan {
    int64_t ws_off[kFMaxLevels];
    int splits[kFMaxLevels], kps[kFMaxLevels], tiles_n[kFMaxLevels], ho[kFMaxLevels], wo[kFMaxLevels];
    int64_t ws_bytes;
};

int make_plan(const char *what, const sdetr_frontend_level *levels, int n_levels, int batch, int out_channels, Plan &pl)
{
    if (!levels || n_levels < 1 || n_levels > kFMaxLevels) return fail("%s: 1..%d levels, got %d", what, kFMaxLevels, n_levels);
    if (batch < 1 || out_channels < 1) return fail("%s: bad batch %d / out_channels %d", what, batch, out_channels);
    const int tiles_m = (out_channels + kFTile - 1) / kFTile;
    int64_t off = 0;
    for (int i = 0; i < n_levels; ++i) {
        const sdetr_frontend_level &L = levels[i];
        if (L.in_channels < 32 || L.in_channels % 32 || L.height < 1 || L.width < 1)
            return fail("%s: level %d: in_channels %d (a multiple of 32) x %d x %d", what, i, L.in_channels, L.height, L.width);
        if (L.kernel_size != 1 && L.kernel_size != 3) return fail("%s: level %d: kernel_size %d (1 or 3)", what, i, L.kernel_size);
        const int ho = L.kernel_size == 1 ? L.height : (L.height - 1) / 2 + 1;
        const int wo = L.kernel_size == 1 ? L.width : (L.width - 1) / 2 + 1;
        const int64_t P = (int64_t)ho * wo, K = (int64_t)L.in_channels * L.kernel_size * L.kernel_size;
        if (P * out_channels > 0x7fffffffLL || K * out_channels > 0x7fffffffLL || (int64_t)L.in_channels * L.height * L.width > 0x7fffffffLL)
            return fail("%s: level %d too large", what, i);
        const int tn = (int)((P + kFTile - 1) / kFTile);
        int splits = 1, kps = (int)K;
        if (L.kernel_size == 3) {   // split K so that the level alone fills ~256 workgroups, >= 256 reduction indices each
            const int tiles = batch * tiles_m * tn;
            splits = std::max(1, std::min(24, (256 + tiles - 1) / tiles));
            kps = (int)(((K + splits - 1) / splits + kFK - 1) / kFK * kFK);
            kps = std::max(kps, std::min((int)K, 256));
            splits = (int)((K + kps - 1) / kps);
        }
        pl.ho[i] = ho; pl.wo[i] = wo; pl.tiles_n[i] = tn; pl.splits[i] = splits; pl.kps[i] = kps;
        pl.ws_off[i] = off;
        off += L.kernel_size == 1 ? (int64_t)batch * out_channels * tn * 2 * 4 : (int64_t)splits * batch * out_channels * P * 4;
        off = (off + 255) / 256 * 256;
    }
    pl.ws_bytes = off;
    return 0;
}

}  // namespace
}  // namespace sdetr

using namespace sdetr;

extern "C" int64_t sdetr_frontend_workspace_bytes(const sdetr_frontend_level *levels, int n_levels, int batch, int out_channels)
{
    Plan pl;
    if (make_plan("frontend_workspace_bytes", levels, n_levels, batch, out_channels, pl)) return -1;
    return pl.ws_bytes;
}

extern "C" int64_t sdetr_frontend_packed_bytes(int64_t count, int precision)
{
    if (count < 0 || (precision != 0 && precision != 1)) return -1;
    return count * (precision == 0 ? 3 : 1) * (int64_t)sizeof(uint16_t);
}

extern "C" int sdetr_frontend_pack_weight(sdetr_stream_t stream, const float *weight, int64_t count, int precision, void *out)
{
    const char *what = "frontend_pack_weight";
    if (!weight || !out || count < 1) return fail("%s: null pointer or empty weight", what);
    if (precision != 0 && precision != 1) return fail("%s: precision %d (0 fp32, 1 16-bit)", what, precision);
    const int64_t blocks = std::min<int64_t>((count + kFThreads - 1) / kFThreads, 4096);
    hipLaunchKernelGGL(frontend_pack_kernel, dim3((unsigned)blocks), dim3(kFThreads), 0, (hipStream_t)stream, weight, count,
                       precision, static_cast<uint16_t *>(out));
    return check_launch(what);
}

extern "C" int sdetr_frontend_conv_splits(const sdetr_frontend_level *levels, int n_levels, int batch, int out_channels,
                                          int *splits, int64_t *workspace_offsets)
{
    Plan pl;
    if (int rc = make_plan("frontend_conv_splits", levels, n_levels, batch, out_channels, pl)) return rc;
    for (int i = 0; i < n_levels; ++i) {
        if (splits) splits[i] = pl.splits[i];
        if (workspace_offsets) workspace_offsets[i] = pl.ws_off[i];
    }
    return 0;
}

extern "C" int sdetr_frontend_conv(sdetr_stream_t stream, const sdetr_frontend_level *levels, int n_levels, int batch,
                                   int out_channels, int precision, void *workspace, int64_t workspace_bytes)
{
    const char *what = "frontend_conv";
    Plan pl;
    if (int rc = make_plan(what, levels, n_levels, batch, out_channels, pl)) return rc;
    if (precision != 0 && precision != 1) return fail("%s: precision %d (0 fp32, 1 16-bit)", what, precision);
    if (!workspace || workspace_bytes < pl.ws_bytes)
        return fail("%s: workspace too small (%lld bytes needed)", what, (long long)pl.ws_bytes);
    ConvArgs a{};
    a.n_levels = n_levels; a.batch = batch; a.co = out_channels; a.precision = precision;
    const int tiles_m = (out_channels + kFTile - 1) / kFTile;
    int64_t blocks = 0;
    for (int i = 0; i < n_levels; ++i) {
        const sdetr_frontend_level &L = levels[i];
        if (!L.x || !L.weight) return fail("%s: level %d: null input or weight", what, i);
        if (L.kernel_size == 1 && !L.out) return fail("%s: level %d: null output", what, i);
        if ((reinterpret_cast<uintptr_t>(L.weight) & 15) || (reinterpret_cast<uintptr_t>(L.x) & 15))
            return fail("%s: level %d: input and weight must be 16-byte aligned", what, i);
        ConvLevel &c = a.lv[i];
        c.x = L.x; c.w = static_cast<const uint16_t *>(L.weight);
        c.plane = (int64_t)out_channels * L.in_channels * L.kernel_size * L.kernel_size;
        char *ws = static_cast<char *>(workspace) + pl.ws_off[i];
        c.out = L.kernel_size == 1 ? L.out : reinterpret_cast<float *>(ws);
        c.stats = reinterpret_cast<float *>(ws);
        c.cin = L.in_channels; c.h = L.height; c.w_in = L.width; c.ho = pl.ho[i]; c.wo = pl.wo[i];
        c.kernel = L.kernel_size; c.K = L.in_channels * L.kernel_size * L.kernel_size; c.P = pl.ho[i] * pl.wo[i];
        c.tiles_n = pl.tiles_n[i]; c.tiles_m = tiles_m; c.splits = pl.splits[i]; c.k_per_split = pl.kps[i];
        c.block0 = (int)blocks;
        blocks += (int64_t)c.splits * batch * tiles_m * c.tiles_n;
        if (blocks > 0x7fffffffLL) return fail("%s: too many tiles", what);
    }
    hipStream_t s = (hipStream_t)stream;
    if (precision == 0) {
        allow_dynamic_lds(frontend_conv_kernel<true>, g_conv_lds_x3, kFLds);
        hipLaunchKernelGGL(frontend_conv_kernel<true>, dim3((unsigned)blocks), dim3(kFThreads), kFLds, s, a);
    } else {
        allow_dynamic_lds(frontend_conv_kernel<false>, g_conv_lds_16, kFLds);
        hipLaunchKernelGGL(frontend_conv_kernel<false>, dim3((unsigned)blocks), dim3(kFThreads), kFLds, s, a);
    }
    return check_launch(what);
}

// the one GroupNorm launch; z / stats (host arrays of n_levels device pointers) make it the training forward's
static int launch_groupnorm(const char *what, sdetr_stream_t stream, const sdetr_frontend_level *levels, int n_levels, int batch,
                            int out_channels, int num_groups, float eps, const void *workspace, int64_t workspace_bytes,
                            float *const *z, float *const *stats)
{
    Plan pl;
    if (int rc = make_plan(what, levels, n_levels, batch, out_channels, pl)) return rc;
    if (num_groups < 1 || out_channels % num_groups)
        return fail("%s: %d channels in %d groups", what, out_channels, num_groups);
    if (!workspace || workspace_bytes < pl.ws_bytes)
        return fail("%s: workspace too small (%lld bytes needed)", what, (long long)pl.ws_bytes);
    NormArgs a{};
    a.n_levels = n_levels; a.batch = batch; a.co = out_channels; a.groups = num_groups; a.eps = eps;
    const int cg = out_channels / num_groups;
    int64_t blocks = 0;
    for (int i = 0; i < n_levels; ++i) {
        const sdetr_frontend_level &L = levels[i];
        if (!L.out || !L.gamma || !L.beta) return fail("%s: level %d: null output or affine", what, i);
        NormLevel &n = a.lv[i];
        n.out = L.out;
        n.part = reinterpret_cast<const float *>(static_cast<const char *>(workspace) + pl.ws_off[i]);
        n.gamma = L.gamma; n.beta = L.beta;
        if (z) {
            if (!z[i] || !stats[i] || z[i] == L.out) return fail("%s: level %d: null z or stats, or z aliases out", what, i);
            n.z = z[i]; n.stats = stats[i];
        }
        n.P = pl.ho[i] * pl.wo[i]; n.kernel = L.kernel_size; n.tiles_n = pl.tiles_n[i]; n.splits = pl.splits[i];
        n.chunks = L.kernel_size == 1 ? (int)(((int64_t)cg * n.P + kFNormChunk - 1) / kFNormChunk) : 1;
        n.block0 = (int)blocks;
        blocks += (int64_t)batch * num_groups * n.chunks;
        if (blocks > 0x7fffffffLL) return fail("%s: too many workgroups", what);
    }
    if (z) hipLaunchKernelGGL(frontend_groupnorm_kernel<true>, dim3((unsigned)blocks), dim3(kFThreads), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(frontend_groupnorm_kernel<false>, dim3((unsigned)blocks), dim3(kFThreads), 0, (hipStream_t)stream, a);
    return check_launch(what);
}

extern "C" int sdetr_frontend_groupnorm(sdetr_stream_t stream, const sdetr_frontend_level *levels, int n_levels, int batch,
                                        int out_channels, int num_groups, float eps, const void *workspace,
                                        int64_t workspace_bytes)
{
    return launch_groupnorm("frontend_groupnorm", stream, levels, n_levels, batch, out_channels, num_groups, eps, workspace,
                            workspace_bytes, nullptr, nullptr);
}

extern "C" int sdetr_frontend_groupnorm_train(sdetr_stream_t stream, const sdetr_frontend_level *levels, int n_levels,
                                              int batch, int out_channels, int num_groups, float eps, const void *workspace,
                                              int64_t workspace_bytes, float *const *z, float *const *stats)
{
    if (!z || !stats) return fail("frontend_groupnorm_train: null z or stats array");
    return launch_groupnorm("frontend_groupnorm_train", stream, levels, n_levels, batch, out_channels, num_groups, eps,
                            workspace, workspace_bytes, z, stats);
}

extern "C" int sdetr_frontend_masks_positions(sdetr_stream_t stream, const uint8_t *mask, int batch, int height, int width,
                                              int n_levels, const int *level_hw, const float *dim_ty, const float *dim_tx,
                                              int num_pos_feats, int normalize, float scale, float eps, float offset,
                                              uint8_t *const *level_masks, float *const *level_pos)
{
    const char *what = "frontend_masks_positions";
    if (!mask || !level_hw || !dim_ty || !dim_tx || !level_masks || !level_pos) return fail("%s: null pointer", what);
    if (batch < 1 || height < 1 || width < 1 || num_pos_feats < 1 || n_levels < 1 || n_levels > kFMaxLevels)
        return fail("%s: bad sizes (batch %d, %d x %d, %d features, %d levels)", what, batch, height, width, num_pos_feats,
                    n_levels);
    PosArgs a{};
    a.src = mask; a.dim_ty = dim_ty; a.dim_tx = dim_tx;
    a.n_levels = n_levels; a.batch = batch; a.H = height; a.W = width; a.F = num_pos_feats; a.normalize = normalize;
    a.scale = scale; a.eps = eps; a.offset = offset;
    int64_t blocks = 0;
    for (int i = 0; i < n_levels; ++i) {
        const int h = level_hw[2 * i], w = level_hw[2 * i + 1];
        if (h < 1 || w < 1 || (int64_t)batch * 2 * num_pos_feats * h * w > 0x7fffffffLL)
            return fail("%s: level %d: bad shape %d x %d", what, i, h, w);
        if (!level_masks[i] || !level_pos[i]) return fail("%s: level %d: null output", what, i);
        a.lv[i] = PosLevel{level_masks[i], level_pos[i], h, w, (int)blocks};
        blocks += ((int64_t)batch * h * w + kFThreads - 1) / kFThreads;
    }
    hipLaunchKernelGGL(frontend_positions_kernel, dim3((unsigned)blocks), dim3(kFThreads), 0, (hipStream_t)stream, a);
    return check_launch(what);
}

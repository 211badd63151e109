// Shared definitions of the salience head kernels and the body of stage 1 on the bf16 matrix cores (see
// salience_head.hip), as a device function so that another launch can carry it next to other work
// (fused_head_value.hip).
#pragma once
#include "common.h"
#include "gelu_core.h"   // erf_pos / gelu_erf (every statement an explicit fmaf or a single operation)

// No implicit mul + add fusion in this header: the body below is compiled into two different kernels (its own launch and
// the one that also carries a value-projection job), and with hipcc's default (-ffp-contract=fast) the two inlining
// contexts fuse different pairs -- last-bit differences in the scores, i.e. different tokens selected depending on
// which launch ran.  Explicit fmaf() calls are unaffected.
#pragma clang fp contract(off)

namespace sdetr {

constexpr int kC = 256;        // embed dim == hidden dim of the head
constexpr int kHalf = 128;
constexpr int kTM = 64;        // tokens per block
constexpr int kXS = kC + 4;    // LDS row stride of the token tile (floats)
constexpr int kZS = kHalf + 4;

using f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ __forceinline__ f32x16 mfma4(const float4 a, const float4 b, f32x16 c)
{
#ifdef SH_KO_F32_MFMA   // (benchmark builds: what the f32 products cost a launch)
    c[0] += a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
    return c;
#endif
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, c, 0, 0, 0);
    return c;
}

// ---- the weight operand -----------------------------------------------------------------------------------
// It comes straight from L2 (every block streams the same 256 KB), so its loads run PD steps (PD * CT KB per wave)
// ahead of the MFMAs that consume them: one step of 4*RT*CT MFMAs is only ~0.1-0.4 us, an L2 hit ~0.5 us and the
// first touch after other kernels flushed the L2 ~2 us.  Buffer loads (uniform base and step offset in SGPRs, one
// lane offset) keep the 16-byte loads whole and cost no address VALU.  The first PD steps are requested by
// start() -- callers do that BEFORE the barrier / LayerNorm phase in front of the GEMM, so the pipeline is already
// full when the MFMAs begin.
template <int CT, int PD>
struct WeightStream {
    __amdgpu_buffer_rsrc_t rs;
    uint32_t lane_off, step;
    u32x4_t bq[PD][CT];

    __device__ __forceinline__ void start(const float4 *wp, int N, int ksteps, int n0, int lane)
    {
        step = (uint32_t)N * 32;   // bytes per k-step of the packed weight
        rs = make_uniform_rsrc(reinterpret_cast<const char *>(wp), step * (uint32_t)ksteps);
        lane_off = (uint32_t)((n0 + (lane & 31)) * 2 + (lane >> 5)) * 16;
#pragma unroll
        for (int u = 0; u < PD; ++u)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
                bq[u][ct] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(lane_off + ct * 1024), (int)(u * step), 0);
    }
};

// acc[rt][ct] += tile[32rt + i][k] * W[n0 + 32ct + j][k]   (tile in LDS with row stride XS; W through `ws`)
template <int KDIM, int XS, int RT, int CT, int PD>
__device__ __forceinline__ void block_gemm(const float *tile, WeightStream<CT, PD> &ws, int lane, f32x16 (&acc)[RT][CT])
{
    constexpr int NS = KDIM / 8;
    static_assert(NS % PD == 0, "prefetch depth must divide the step count");
    const float *ap = tile + (lane & 31) * XS + 4 * (lane >> 5);
    // fully unrolled: a rolled loop carries the in-flight registers across the back edge through copies, and
    // every copy waits for its load (the pipeline would drain once per PD steps)
#pragma unroll
    for (int S0 = 0; S0 < NS; S0 += PD) {
#pragma unroll
        for (int u = 0; u < PD; ++u) {
            const int S = S0 + u;
            u32x4_t b[CT];
            float4 a[RT];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) b[ct] = ws.bq[u][ct];
            if (S + PD < NS) {
#pragma unroll
                for (int ct = 0; ct < CT; ++ct)
                    ws.bq[u][ct] = __builtin_amdgcn_raw_buffer_load_b128(ws.rs, (int)(ws.lane_off + ct * 1024),
                                                                         (int)((S + PD) * ws.step), 0);
            }
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) a[rt] = *reinterpret_cast<const float4 *>(ap + rt * 32 * XS + 8 * S);
            // pin this step's prefetch in front of its MFMAs (the scheduler otherwise sinks the loads next to
            // their uses, which serialises every step on L2 latency)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    const float4 bf = make_float4(__uint_as_float(b[ct].x), __uint_as_float(b[ct].y),
                                                  __uint_as_float(b[ct].z), __uint_as_float(b[ct].w));
                    acc[rt][ct] = mfma4(a[rt], bf, acc[rt][ct]);
                }
        }
    }
}

template <int RT, int CT>
__device__ __forceinline__ void zero_acc(f32x16 (&acc)[RT][CT])
{
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[rt][ct][i] = 0.f;
}

// row of accumulator register `reg` inside a 32x32 tile
__device__ __forceinline__ int acc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

struct Stage1Args {
    const float *x;            // [B, n, 256] with strides
    int64_t x_batch_stride, x_row_stride;
    const float4 *w_enc;       // packed enc_output weight or NULL (x is already enc_output_norm's output)
    const float *b_enc, *g_enc, *beta_enc;
    float eps_enc;
    const float *row_scale;    // [B, n] or NULL
    const float *coarse;       // [B, ch, cw] coarser score map or NULL
    int ch, cw, h, w;
    const float *alpha;        // device scalar (NULL = 1)
    const float *g1, *beta1;
    float eps1;
    const float4 *w1;          // packed layer1 Linear weight
    const float *b1;
    float *memory_out;         // enc_output_norm output [B, n, 256] (batch stride given) or NULL
    int64_t mem_batch_stride;
    float *z_local;            // [B, n, 128]
    float *partial;            // [B, nblk, 128]
    int n, nblk;
    // HOISTED form (g_out != NULL; round 6): everything of stage 1 that does not depend on the coarser level's score, for
    // ALL levels' tokens in one launch.  The modulation is a per-token scalar s, and LayerNorm of a scaled row is the
    // unscaled row's times a scalar: with mu, sigma^2 the statistics of the row x,
    //     LN(s x) = k gamma (x - mu) / sigma + beta,   k = s sigma / sqrt(s^2 sigma^2 + eps)
    //     layer1.Linear(LN(s x)) = k G + c0,   G = W (gamma (x - mu) / sigma),   c0 = W beta + b.
    // This launch writes G and sigma; per level only `modulate_body` (resize -> s -> k -> GELU -> halves) is left in the
    // coarse-to-fine chain.  No row_scale / coarse, no z_local / partial.
    float *g_out = nullptr;    // [B, n, 256], images g_batch_stride apart
    int64_t g_batch_stride = 0;
    float *sigma_out = nullptr;   // [B, n], images sigma_batch_stride apart
    int64_t sigma_batch_stride = 0;
};

// sum over the TPR (a power of two <= 16... or more) lanes of a row, the xor butterfly s[i] += s[i ^ o], o = 1, 2, 4, ...
// For TPR == 16 the steps are DPP moves inside the vector ALU (round 6; same partners, same bits as the shuffles: xor 1
// and 2 are quad permutations, xor 4 = half-row mirror (i ^ 7) then reversed quads (i ^ 3), xor 8 = rotation by 8 in
// the row of 16) instead of four ds_bpermute -- each a round trip through the LDS queue, behind the fragment reads of the
// CU's other workgroup: cycle stamps put the LayerNorm phase at 4 900 cycles on an empty chip and 11 000-15 000 in the
// finest level's launch.
template <int TPR>
__device__ __forceinline__ float row_sum(float s)
{
#ifndef SH_SHUFFLE_STATS
    if (TPR == 16) {
        s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0xB1, 0xf, 0xf, true));    // quad_perm [1,0,3,2]
        s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x4E, 0xf, 0xf, true));    // quad_perm [2,3,0,1]
        const int t = __builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x141, 0xf, 0xf, true);          // row_half_mirror
        s += __int_as_float(__builtin_amdgcn_update_dpp(0, t, 0x1B, 0xf, 0xf, true));                    // quad_perm [3,2,1,0]
        s += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x128, 0xf, 0xf, true));   // row_ror:8
        return s;
    }
#endif
#pragma unroll
    for (int o = 1; o < TPR; o <<= 1) s += __shfl_xor(s, o, TPR);
    return s;
}

// two-pass LayerNorm statistics of a row held as NV float4 per thread by the TPR threads of the row
template <int NV, int TPR>
__device__ __forceinline__ void row_stats(const float4 (&v)[NV], float eps, float &mean, float &rstd)
{
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    s = row_sum<TPR>(s);
    mean = s * (1.f / kC);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
        q += (a * a + b * b) + (c * c + d * d);
    }
    q = row_sum<TPR>(q);
    rstd = rsqrtf(q * (1.f / kC) + eps);
}

__device__ __forceinline__ float4 ln_apply(float4 v, float mean, float rstd, float4 g, float4 be)
{
    return make_float4((v.x - mean) * rstd * g.x + be.x, (v.y - mean) * rstd * g.y + be.y,
                       (v.z - mean) * rstd * g.z + be.z, (v.w - mean) * rstd * g.w + be.w);
}

// LDS parameter rows
enum { kParBEnc = 0, kParGEnc, kParBetaEnc, kParG1, kParBeta1, kParB1, kParRows };

// RT = row tiles of 32 tokens per block: 2 halves the weight traffic per token, 1 doubles the blocks (more CUs
// busy on the small levels, finer load balance on the big one; four blocks fit a CU).
// Blocks that share a CU start together and stay in lock step (same work), so nothing hides the phases between
// the two GEMMs except what the block overlaps itself: every global read of those phases (LayerNorm parameters,
// biases, the coarse score for the resize, alpha) is issued up front into LDS together with the token tile, and
// each GEMM's first weight steps are requested before the barrier / LayerNorm phase in front of it.

// ------------------------------------------------------------------------------------------------------------
// Stage 1 on the bf16 matrix cores at fp32 accuracy ("bf16 x 3").  The fp32-input MFMA of the kernel above runs at
// 157 TFLOP/s and the two 256 x 256 GEMMs keep it busy for half of the kernel's time (profiles/r02_mfma_busy.md);
// v_mfma_f32_32x32x16_bf16 is 16 times faster per multiply-add.  Every fp32 operand is split exactly into three
// bf16 terms, x = x0 + x1 + x2 (24 mantissa bits = 3 x 8), and the product a.b is taken as the six bf16 MFMAs
// a0b0 + a0b1 + a1b0 + a1b1 + a0b2 + a2b0: each bf16 x bf16 product is exact in fp32, accumulation is fp32 as before,
// and the dropped terms (a1b2, a2b1, a2b2) are below 2^-24 of the product -- the rounding the fp32 MFMA makes on the
// product itself.  6/16 of the matrix time for the same scores (tests/test_filter_gpu.py compares both kernels with
// the oracle; the selection is identical).  Weights are split once at pack time (sdetr_pack_linear_bf16x3: three
// planes in operand order, [k-step of 16][32-column tile][plane][lane][8]); the token tile is split once per GEMM
// into three LDS planes (the split costs 8 VALU operations per element: done per wave on its operand fragments it
// would cost more than the MFMAs it feeds).
typedef __bf16 sh_bf16x8_t __attribute__((ext_vector_type(8)));
// k-steps of weight (3 KB per wave and step) in flight: a step's six MFMAs take ~0.09 us, an L2 hit ~0.5-0.8 us
constexpr int kX3Depth = 5;
constexpr int kPlaneRow = kC * 2 + 16;                 // bytes per token row of a plane (16 bytes of padding)
constexpr int kPlaneBytes = 32 * kPlaneRow;            // 32-token tile
constexpr int kX3Region = 3 * kPlaneBytes;             // 50 688 bytes: three planes, or the fp32 tile (33 280)
static_assert(kX3Region >= 32 * kXS * 4, "the fp32 tile aliases the planes");

__device__ __forceinline__ f32x16 mfma_bf16(u32x4_t a, u32x4_t b, f32x16 c)
{
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(sh_bf16x8_t, a), __builtin_bit_cast(sh_bf16x8_t, b), c, 0, 0, 0);
}

// exact three-way split of four consecutive elements -> 4 bf16 of each plane.  Round 6: the three roundings through the
// hardware's packed converter (v_cvt_pk_bf16_f32: round-to-nearest-even, the rule of f32_to_bf16_bits -- same bits) instead
// of three software roundings per element: the residuals x - h and (x - h) - m are exact in fp32 either way.
template <bool SOFT>
__device__ __forceinline__ void split3(const float4 v, uint2 &p0, uint2 &p1, uint2 &p2)
{
    if (SOFT) {
    const float x[4] = {v.x, v.y, v.z, v.w};
    uint32_t h[4], m[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        h[i] = f32_to_bf16_bits(x[i]);
        const float r1 = x[i] - __uint_as_float(h[i] << 16);
        m[i] = f32_to_bf16_bits(r1);
        const float r2 = r1 - __uint_as_float(m[i] << 16);
        l[i] = f32_to_bf16_bits(r2);
    }
    p0 = make_uint2(h[0] | (h[1] << 16), h[2] | (h[3] << 16));
    p1 = make_uint2(m[0] | (m[1] << 16), m[2] | (m[3] << 16));
    p2 = make_uint2(l[0] | (l[1] << 16), l[2] | (l[3] << 16));
    return;
    }
    const uint32_t h01 = pack_bf16x2(v.x, v.y), h23 = pack_bf16x2(v.z, v.w);
    const float r0 = v.x - bf16_lo(h01), r1 = v.y - bf16_hi(h01), r2 = v.z - bf16_lo(h23), r3 = v.w - bf16_hi(h23);
    const uint32_t m01 = pack_bf16x2(r0, r1), m23 = pack_bf16x2(r2, r3);
    const float s0 = r0 - bf16_lo(m01), s1 = r1 - bf16_hi(m01), s2 = r2 - bf16_lo(m23), s3 = r3 - bf16_hi(m23);
    p0 = make_uint2(h01, h23);
    p1 = make_uint2(m01, m23);
    p2 = make_uint2(pack_bf16x2(s0, s1), pack_bf16x2(s2, s3));
}
template <bool SOFT = false>
__device__ __forceinline__ void store_split(char *planes, int row, int col, const float4 v)
{
    uint2 p0, p1, p2;
    split3<SOFT>(v, p0, p1, p2);
    char *d = planes + row * kPlaneRow + col * 2;
    *reinterpret_cast<uint2 *>(d) = p0;
    *reinterpret_cast<uint2 *>(d + kPlaneBytes) = p1;
    *reinterpret_cast<uint2 *>(d + 2 * kPlaneBytes) = p2;
}

// the split weight of one wave's 32-column tile, PD k-steps (3 KB each) ahead of the MFMAs
template <int PD>
struct WeightStreamX3 {
    __amdgpu_buffer_rsrc_t rs;
    uint32_t lane_off;
    u32x4_t bq[PD][3];
    static constexpr uint32_t kStep = 8 * 3 * 1024;   // bytes per k-step: 8 column tiles x 3 planes x 1 KB

    __device__ __forceinline__ void start(const void *wp, int ctile, int lane)
    {
        rs = make_uniform_rsrc(reinterpret_cast<const char *>(wp), kStep * (kC / 16));
        lane_off = (uint32_t)(ctile * 3 * 1024 + lane * 16);
#pragma unroll
        for (int u = 0; u < PD; ++u)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                bq[u][pl] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(lane_off + pl * 1024), (int)(u * kStep), 0);
    }
};

// acc += tile[32][256] (three planes in LDS) * W[my 32 columns][256]^T
template <int PD>
__device__ __forceinline__ void block_gemm_x3(const char *planes, WeightStreamX3<PD> &ws, int lane, f32x16 &acc)
{
    constexpr int NS = kC / 16;
    const char *ap = planes + (lane & 31) * kPlaneRow + (lane >> 5) * 16;
    // fully unrolled, the PD in-flight steps live in a ring indexed at compile time (see block_gemm)
#pragma unroll
    for (int S = 0; S < NS; ++S) {
        const int u = S % PD;
        u32x4_t b[3], a[3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) b[pl] = ws.bq[u][pl];
        if (S + PD < NS) {
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                ws.bq[u][pl] = __builtin_amdgcn_raw_buffer_load_b128(ws.rs, (int)(ws.lane_off + pl * 1024),
                                                                     (int)((S + PD) * ws.kStep), 0);
        }
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) a[pl] = *reinterpret_cast<const u32x4_t *>(ap + pl * kPlaneBytes + S * 32);
        __builtin_amdgcn_sched_barrier(0);   // this step's prefetch stays in front of its MFMAs (see block_gemm)
        acc = mfma_bf16(a[2], b[0], acc);    // smallest terms first
        acc = mfma_bf16(a[0], b[2], acc);
        acc = mfma_bf16(a[1], b[1], acc);
        acc = mfma_bf16(a[1], b[0], acc);
        acc = mfma_bf16(a[0], b[1], acc);
        acc = mfma_bf16(a[0], b[0], acc);
    }
}

// The same for other shapes (round 6: stage 2's first product): NT column tiles of 32 in the packed weight, the operand
// planes ROWS x KDIM (row stride KDIM * 2 + 16 bytes), RT row tiles of 32 per wave.
template <int NT, int PD>
struct WeightStreamX3G {
    __amdgpu_buffer_rsrc_t rs;
    uint32_t lane_off;
    u32x4_t bq[PD][3];
    static constexpr uint32_t kStep = NT * 3 * 1024;   // bytes per k-step: NT column tiles x 3 planes x 1 KB

    __device__ __forceinline__ void start(const void *wp, int ksteps, int ctile, int lane)
    {
        rs = make_uniform_rsrc(reinterpret_cast<const char *>(wp), kStep * (uint32_t)ksteps);
        lane_off = (uint32_t)(ctile * 3 * 1024 + lane * 16);
#pragma unroll
        for (int u = 0; u < PD; ++u)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                bq[u][pl] = __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(lane_off + pl * 1024), (int)(u * kStep), 0);
    }
};
template <int KDIM, int ROWS, int RT, int NT, int PD>
__device__ __forceinline__ void block_gemm_x3g(const char *planes, WeightStreamX3G<NT, PD> &ws, int lane, f32x16 (&acc)[RT])
{
    constexpr int NS = KDIM / 16, kRow = KDIM * 2 + 16, kPlane = ROWS * kRow;
    const char *ap = planes + (lane & 31) * kRow + (lane >> 5) * 16;
#pragma unroll
    for (int S = 0; S < NS; ++S) {
        const int u = S % PD;
        u32x4_t b[3], a[RT][3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) b[pl] = ws.bq[u][pl];
        if (S + PD < NS) {
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                ws.bq[u][pl] = __builtin_amdgcn_raw_buffer_load_b128(ws.rs, (int)(ws.lane_off + pl * 1024),
                                                                     (int)((S + PD) * ws.kStep), 0);
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                a[rt][pl] = *reinterpret_cast<const u32x4_t *>(ap + rt * 32 * kRow + pl * kPlane + S * 32);
        __builtin_amdgcn_sched_barrier(0);   // this step's prefetch stays in front of its MFMAs (see block_gemm)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            acc[rt] = mfma_bf16(a[rt][2], b[0], acc[rt]);    // smallest terms first
            acc[rt] = mfma_bf16(a[rt][0], b[2], acc[rt]);
            acc[rt] = mfma_bf16(a[rt][1], b[1], acc[rt]);
            acc[rt] = mfma_bf16(a[rt][1], b[0], acc[rt]);
            acc[rt] = mfma_bf16(a[rt][0], b[1], acc[rt]);
            acc[rt] = mfma_bf16(a[rt][0], b[0], acc[rt]);
        }
    }
}
// stage 2's token tile as planes: 64 rows x 128 values
constexpr int kS2PlaneRow = kHalf * 2 + 16;            // 272 bytes
constexpr int kS2PlaneBytes = 64 * kS2PlaneRow;        // 17 408
constexpr int kS2Planes = 3 * kS2PlaneBytes;           // 52 224

// ---- stage 1 straight from the pyramid (PYR form of stage1_x3_body) ---------------------------------------------------
// The hoisted launch used to read enc_in = keep ? feat + (pos + level_embed) : 0 back from memory, 45.7 MB of fp32 rows
// that pyramid_flatten_all_kernel (plumbing.hip) had written one launch earlier for this reader alone.  In the PYR form
// the workgroup builds its 32 rows of enc_in itself from the fp32 NCHW maps -- the same keep rule, the same two fp32
// additions, the same bits -- and writes what the flatten wrote for the REST of the step: the 16-bit copies of feat and
// pos + level_embed, the flattened padding mask, the valid ratios.  Tiles are dealt over the flat token index of an image,
// so a tile can straddle image rows and levels: every token row resolves its own level / y / x (one integer division per
// row, by the 32 threads that also fetch the row's padding byte); the loads themselves need the offset inside the level only.
constexpr int kPyrMaxLevels = 8;
constexpr int kPyrTileLevels = 4;   // levels one 32-token tile may touch (the launcher checks)
struct PyramidSrc {
    const float *feat[kPyrMaxLevels], *pos[kPyrMaxLevels];   // fp32 [B, 256, H, W] per level
    const uint8_t *mask[kPyrMaxLevels];                       // [B, H, W], non-zero = padding
    int H[kPyrMaxLevels], W[kPyrMaxLevels], start[kPyrMaxLevels + 1];
    float box_wh[kPyrMaxLevels];                              // 0.05 * 2^level (the proposal's box side)
    const float *level_embed;                                 // [levels, 256]
    int levels;
    bf16_t *feat_act, *pos_act;                               // [B, S, 256] 16-bit activations
    uint8_t *mask_out;                                        // [B, S]
    float *valid_ratios;                                      // [B, levels, 2] (w, h) or NULL
};
// LDS of the PYR form (floats): feat tile | pos tile | parameter rows | srow | level embeddings | level geometry | row info
constexpr int kPyrGeo = 8;          // per touched level: valid height, valid width, H, W, box_wh
constexpr int kPyrLdsFloats = 2 * 32 * kXS + kParRows * kC + 32 + 4 + kPyrTileLevels * kC + kPyrTileLevels * kPyrGeo + 32 * 4;

// (`blk` / `b` = token block and image: the kernel's own block indices, or the position inside a launch that also
// carries other work -- fused_head_value.hip.  The first 512 threads of the workgroup take part.)
template <bool PYR = false>
__device__ __forceinline__ void stage1_x3_body(const Stage1Args &p, int blk, int b, const PyramidSrc *src = nullptr)
{
    constexpr int TM = 32, THREADS = 512;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char *planes = reinterpret_cast<char *>(smem);               // three bf16 planes of the GEMM operand ...
    float *tile = smem;                                           // ... or the fp32 tile [TM][kXS] between the GEMMs
    float *par = smem + (PYR ? 2 * TM * kXS : kX3Region / 4);    // [kParRows][kC] (PYR: behind the feat and pos tiles)
    float *srow = par + kParRows * kC;                            // [TM] modulation factor, [TM] = alpha
    float *tpos = smem + TM * kXS;                                // PYR: the position tile [TM][kXS] next to the feature tile
    float *lemb = srow + TM + 4;                                  // PYR: [kPyrTileLevels][kC] level embeddings of the tile's levels
    float *geo = lemb + kPyrTileLevels * kC;                      // PYR: [kPyrTileLevels][kPyrGeo]
    int *rowinfo = reinterpret_cast<int *>(geo + kPyrTileLevels * kPyrGeo);   // PYR: [TM][4] level slot, x, y, padding
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t0 = blk * TM;
    const int nvalid = min(TM, p.n - t0);
    const int n0 = wave * 32;
    const bool with_enc = p.w_enc != nullptr;
    const bool hoist = p.g_out != nullptr;

    // (benchmark builds only, -DSH_STAMPS through benchmarks/lib_variant.sh: cycle stamps per phase, printed by three
    // workgroups of a launch)
#ifdef SH_STAMPS
    long long sh_t[8];
    int sh_n = 0;
#define SH_STAMP() sh_t[sh_n++] = clock64()
#else
#define SH_STAMP()
#endif
    SH_STAMP();
    WeightStreamX3<kX3Depth> ws;
    ws.start(with_enc ? (const void *)p.w_enc : (const void *)p.w1, wave, lane);

    int l0 = 0;   // PYR: level of the tile's first token
    // ---- token tile (split into planes when a GEMM consumes it directly), parameters and row factors -> LDS ----
    {
        constexpr int NL = TM * 64 / THREADS;   // float4 per thread
        float4 v[NL];
        // PYR: lane = token (32 consecutive tokens of a channel are one 128-byte run of the NCHW map), 16 channels per thread
        constexpr int NC = kC * TM / THREADS;
        float pf[NC], pq[NC];
        const int tok = tid & 31, cg = tid >> 5;
        if (PYR) {
            const PyramidSrc &s = *src;
            for (int j = 1; j < s.levels; ++j) l0 += t0 >= s.start[j] ? 1 : 0;   // level of the tile's first token (uniform)
            const int t = min(t0 + tok, p.n - 1);
            int slot = 0, wl = s.W[l0], hw = s.H[l0] * s.W[l0], st = s.start[l0];
            const float *fp = s.feat[l0], *pp = s.pos[l0];
            const uint8_t *mp = s.mask[l0];
#pragma unroll
            for (int k = 1; k < kPyrTileLevels; ++k) {
                const int l = min(l0 + k, s.levels - 1);
                if (l0 + k < s.levels && t >= s.start[l]) {
                    slot = k; wl = s.W[l]; hw = s.H[l] * s.W[l]; st = s.start[l];
                    fp = s.feat[l]; pp = s.pos[l]; mp = s.mask[l];
                }
            }
            const int tl = t - st;   // the token's pixel inside its level
            const int64_t e0 = ((int64_t)b * kC + cg) * hw + tl;
#pragma unroll
            for (int i = 0; i < NC; ++i) pf[i] = fp[e0 + (int64_t)(i * (THREADS / TM)) * hw];
#pragma unroll
            for (int i = 0; i < NC; ++i) pq[i] = pp[e0 + (int64_t)(i * (THREADS / TM)) * hw];
            if (tid < TM) {   // the row's place in its level: the one division per token row
                const int y = tl / wl;
                *reinterpret_cast<int4 *>(rowinfo + 4 * tok) = make_int4(slot, tl - y * wl, y, (int)mp[(int64_t)b * hw + tl]);
            }
            // valid extents of the touched levels, recounted from column 0 / row 0 of the mask as the flatten does:
            // wave 2k counts level l0 + k's height, wave 2k + 1 its width
            {
                const int l = l0 + (wave >> 1);
                if (l < s.levels && s.start[l] < t0 + TM) {
                    const int H = s.H[l], W = s.W[l];
                    const uint8_t *mb = s.mask[l] + (int64_t)b * H * W;
                    int cnt = 0;
                    if (wave & 1) { for (int i = lane; i < W; i += 64) cnt += mb[i] == 0; }
                    else          { for (int i = lane; i < H; i += 64) cnt += mb[(int64_t)i * W] == 0; }
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
                    if (lane == 0) {
                        float *g = geo + (wave >> 1) * kPyrGeo;
                        g[wave & 1] = (float)cnt;
                        if (!(wave & 1)) { g[2] = (float)H; g[3] = (float)W; g[4] = s.box_wh[l]; }
                    }
                }
            }
            if (tid >= 256) {   // the level embeddings of the tile's levels
                const int l = l0 + ((tid - 256) >> 6), c4 = tid & 63;
                if (l < s.levels)
                    *reinterpret_cast<float4 *>(lemb + ((tid - 256) >> 6) * kC + c4 * 4) =
                        *reinterpret_cast<const float4 *>(s.level_embed + (int64_t)l * kC + c4 * 4);
            }
        } else {
        const float *xb = p.x + (int64_t)b * p.x_batch_stride + (int64_t)t0 * p.x_row_stride;
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int idx = tid + i * THREADS;
            const int r = idx >> 6, c4 = idx & 63;
            v[i] = *reinterpret_cast<const float4 *>(xb + (int64_t)min(r, nvalid - 1) * p.x_row_stride + c4 * 4);
        }
        }
        if (tid < 256) {
            const int row = tid >> 6, c4 = tid & 63;
            const float *src0 = row == 0 ? p.b_enc : row == 1 ? p.g_enc : row == 2 ? p.beta_enc : p.g1;
            const float *src1 = row == 0 ? p.beta1 : p.b1;
            if (with_enc || row == 3) *reinterpret_cast<float4 *>(par + row * kC + c4 * 4) =
                                          *reinterpret_cast<const float4 *>(src0 + c4 * 4);
            if (row < 2) *reinterpret_cast<float4 *>(par + (4 + row) * kC + c4 * 4) =
                             *reinterpret_cast<const float4 *>(src1 + c4 * 4);
        }
        if (tid < TM) {
            float s = 0.f;
            const int t = min(t0 + tid, p.n - 1);
            if (p.row_scale) {
                s = p.row_scale[(int64_t)b * p.n + t];
            } else if (p.coarse) {
                // bilinear, align_corners=True (F.interpolate, salience_transformer.py:139-142)
                const int y = t / p.w, x = t - y * p.w;
                const float sh = p.h > 1 ? (float)(p.ch - 1) / (float)(p.h - 1) : 0.f;
                const float sw = p.w > 1 ? (float)(p.cw - 1) / (float)(p.w - 1) : 0.f;
                const float fy = sh * (float)y, fx = sw * (float)x;
                const int y1 = (int)fy, x1 = (int)fx;
                const int yp = y1 < p.ch - 1 ? 1 : 0, xp = x1 < p.cw - 1 ? 1 : 0;
                const float ly = fy - (float)y1, lx = fx - (float)x1;
                const float hy = 1.f - ly, hx = 1.f - lx;
                const float *cm = p.coarse + (int64_t)b * p.ch * p.cw;
                s = hy * (hx * cm[y1 * p.cw + x1] + lx * cm[y1 * p.cw + x1 + xp]) +
                    ly * (hx * cm[(y1 + yp) * p.cw + x1] + lx * cm[(y1 + yp) * p.cw + x1 + xp]);
            }
            srow[tid] = s;
            if (tid == 0) srow[TM] = (p.row_scale || p.coarse) ? (p.alpha ? *p.alpha : 1.f) : 0.f;
        }
        if (PYR) {   // the transposition: [channel][token] registers -> [token][channel] tiles
#pragma unroll
            for (int i = 0; i < NC; ++i) {
                tile[tok * kXS + cg + i * (THREADS / TM)] = pf[i];
                tpos[tok * kXS + cg + i * (THREADS / TM)] = pq[i];
            }
        }
#pragma unroll
        for (int i = 0; i < (PYR ? 0 : NL); ++i) {
            const int idx = tid + i * THREADS;
            const int r = idx >> 6, c4 = idx & 63;
            const float4 val = r < nvalid ? v[i] : make_float4(0.f, 0.f, 0.f, 0.f);
#ifndef SH_SITE1_SOFT
#define SH_SITE1_SOFT false
#endif
#ifndef SH_SITE2_SOFT
#define SH_SITE2_SOFT false
#endif
            if (with_enc) store_split<SH_SITE1_SOFT>(planes, r, c4 * 4, val);
            else *reinterpret_cast<float4 *>(tile + r * kXS + c4 * 4) = val;
        }
    }
#ifdef SH_STAMPS
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    const long long sh_tile_done = clock64();   // (wave 0: its loads are back, its part of the tile is stored)
#endif
    if (PYR) {
        // ---- rows: 16 threads per token, each 4 float4 of its channels (the LayerNorm phase's mapping): the flatten's outputs
        // of the row, then enc_in's row -- (feat + (pos + level_embed)) * keep, pyramid_flatten_body's arithmetic -- into the planes
        __syncthreads();
        const PyramidSrc &s = *src;
        const int r = tid >> 4, q = tid & 15;
        const int4 ri = *reinterpret_cast<const int4 *>(rowinfo + 4 * r);   // level slot, x, y, padding
        const float *g = geo + ri.x * kPyrGeo;
        const float vh = g[0], vw = g[1], box_wh = g[4];
        const bool pad = ri.w != 0;
        const float cx = ((float)ri.y + 0.5f) / vw, cy = ((float)ri.z + 0.5f) / vh;
        const bool keep = !pad && cx > 0.01f && cx < 0.99f && cy > 0.01f && cy < 0.99f && box_wh > 0.01f && box_wh < 0.99f;
        const bool live = r < nvalid;
        const int64_t o = ((int64_t)b * p.n + t0 + r) * kC + 4 * q;
        float4 sum[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 64 * i + 4 * q;
            const float4 fv = *reinterpret_cast<const float4 *>(tile + r * kXS + c);
            const float4 pv = *reinterpret_cast<const float4 *>(tpos + r * kXS + c);
            const float4 e = *reinterpret_cast<const float4 *>(lemb + ri.x * kC + c);
            const float4 qv = make_float4(pv.x + e.x, pv.y + e.y, pv.z + e.z, pv.w + e.w);
            sum[i] = keep && live ? make_float4(fv.x + qv.x, fv.y + qv.y, fv.z + qv.z, fv.w + qv.w)
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
            if (live) {
                *reinterpret_cast<uint2 *>(s.feat_act + o + 64 * i) = make_uint2(pack_act2(fv.x, fv.y), pack_act2(fv.z, fv.w));
                *reinterpret_cast<uint2 *>(s.pos_act + o + 64 * i) = make_uint2(pack_act2(qv.x, qv.y), pack_act2(qv.z, qv.w));
            }
        }
        if (live && q == 0) {
            s.mask_out[(int64_t)b * p.n + t0 + r] = pad ? 1 : 0;
            if (s.valid_ratios && ri.y == 0 && ri.z == 0) {   // the level's first token: get_valid_ratios, (w, h)
                float *vr = s.valid_ratios + ((int64_t)b * s.levels + l0 + ri.x) * 2;
                vr[0] = vw / g[3];
                vr[1] = vh / g[2];
            }
        }
        __syncthreads();   // every thread holds its part of the two tiles: the planes may overwrite them
#pragma unroll
        for (int i = 0; i < 4; ++i) store_split<SH_SITE1_SOFT>(planes, r, 64 * i + 4 * q, sum[i]);
    }
    __syncthreads();
    SH_STAMP();   // 1: tile, parameters, row factors in LDS

    f32x16 acc;
    if (with_enc) {
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        block_gemm_x3<kX3Depth>(planes, ws, lane, acc);
        SH_STAMP();   // 2: first product
        ws.start(p.w1, wave, lane);   // layer1's first steps travel during the LayerNorm phase
        __syncthreads();   // every wave is done reading the planes: the fp32 tile takes their place
        const int c = n0 + (lane & 31);
        const float bias = par[kParBEnc * kC + c];
#pragma unroll
        for (int i = 0; i < 16; ++i) tile[acc_row(i, lane) * kXS + c] = acc[i] + bias;
        __syncthreads();
        SH_STAMP();   // 3: product + bias back in LDS as fp32
    }

    // ---- enc_output_norm -> modulation -> layer1 LayerNorm; 16 threads per row, each 4 float4; result -> planes ----
    {
        constexpr int TPR = THREADS / TM, NV = kC / 4 / TPR, CS = 4 * TPR;
        const int r = tid / TPR, q = tid % TPR;
        const float *row = tile + r * kXS + 4 * q;
        float4 v[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = *reinterpret_cast<const float4 *>(row + CS * i);
        float mean, rstd;
        if (with_enc) {
            row_stats<NV, TPR>(v, p.eps_enc, mean, rstd);
#pragma unroll
            for (int i = 0; i < NV; ++i)
                v[i] = ln_apply(v[i], mean, rstd, *reinterpret_cast<const float4 *>(par + kParGEnc * kC + CS * i + 4 * q),
                                *reinterpret_cast<const float4 *>(par + kParBetaEnc * kC + CS * i + 4 * q));
            if (p.memory_out && r < nvalid) {
                float *mo = p.memory_out + (int64_t)b * p.mem_batch_stride + (int64_t)(t0 + r) * kC + 4 * q;
#pragma unroll
                for (int i = 0; i < NV; ++i) *reinterpret_cast<float4 *>(mo + CS * i) = v[i];
            }
        }
        const float s = srow[r], a = srow[TM];
        if (a != 0.f) {
#pragma unroll
            for (int i = 0; i < NV; ++i)
                v[i] = make_float4(v[i].x + v[i].x * s * a, v[i].y + v[i].y * s * a, v[i].z + v[i].z * s * a,
                                   v[i].w + v[i].w * s * a);
        }
        // (hoisted: eps = 0 -- the statistics of the row itself; rstd = 1 / sigma, and a constant row gives G = 0)
        row_stats<NV, TPR>(v, hoist ? 0.f : p.eps1, mean, rstd);
        if (hoist) {
            const bool flat = !(rstd < 3.0e38f);   // sigma == 0 (rsqrt(0) = inf)
            if (q == 0 && r < nvalid) p.sigma_out[(int64_t)b * p.sigma_batch_stride + t0 + r] = flat ? 0.f : 1.f / rstd;
            if (flat) rstd = 0.f;
        }
        // The statistics are COMPLETE in front of the barrier below (round 6).  Left to the scheduler, the last step of the
        // 16-lane sum (a ds_bpermute) was issued in front of the barrier and consumed behind it -- and with the faster
        // split of this round that schedule produced wrong rows in ~20 of 33 400 tokens per launch, always in lanes 48-63
        // of a wave, different ones every run (benchmarks/head_determinism.py; cause not found: no hazard the ISA
        // documents; 0 of 400 runs differ with the statistics pinned here, and with the old split).  tests/
        // test_filter_ops_gpu.py::test_salience_head_is_deterministic keeps watch.
#ifndef SH_NO_PIN_STATS
        asm volatile("" : "+v"(mean), "+v"(rstd));
#endif
#pragma unroll
        for (int i = 0; i < NV; ++i)
            v[i] = ln_apply(v[i], mean, rstd, *reinterpret_cast<const float4 *>(par + kParG1 * kC + CS * i + 4 * q),
                            hoist ? make_float4(0.f, 0.f, 0.f, 0.f)
                                  : *reinterpret_cast<const float4 *>(par + kParBeta1 * kC + CS * i + 4 * q));
        // (and the LDS queue is drained, nothing moved across, before the barrier: whatever the schedule in front of this
        // point -- the PYR form changes it -- no LDS result is consumed behind a barrier it was requested in front of)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();   // every thread holds its part of the tile in registers: the planes may overwrite it
#pragma unroll
        for (int i = 0; i < NV; ++i) store_split<SH_SITE2_SOFT>(planes, r, CS * i + 4 * q, v[i]);
    }
    __syncthreads();
    SH_STAMP();   // 4: two LayerNorms + modulation, planes of the second product's operand

    // ---- layer1 Linear + GELU ----
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    block_gemm_x3<kX3Depth>(planes, ws, lane, acc);
    SH_STAMP();   // 5: second product
    if (hoist) {
        // G as it leaves the accumulators (no bias, no GELU): lane = column, 16 rows
        const int c = n0 + (lane & 31);
        float *g = p.g_out + (int64_t)b * p.g_batch_stride + (int64_t)t0 * kC + c;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int r = acc_row(i, lane);
            if (r < nvalid) g[(int64_t)r * kC] = acc[i];
        }
    } else {
        const int c = n0 + (lane & 31);
        const float bias = par[kParB1 * kC + c];
        if (n0 < kHalf) {
            float *zl = p.z_local + ((int64_t)b * p.n + t0) * kHalf;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int r = acc_row(i, lane);
                if (r < nvalid) zl[(int64_t)r * kHalf + c] = gelu_erf(acc[i] + bias);
            }
        } else {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) s += acc_row(i, lane) < nvalid ? gelu_erf(acc[i] + bias) : 0.f;
            s += __shfl_xor(s, 32);
            if (lane < 32) p.partial[((int64_t)b * p.nblk + blk) * kHalf + (c - kHalf)] = s;
        }
    }
#ifdef SH_STAMPS
    SH_STAMP();   // 6: GELU + stores
    if (with_enc && tid == 0 && b == 0 && (blk == 0 || blk == p.nblk / 2 || blk == p.nblk - 1))
        printf("stage1 n=%d blk=%d cycles: (own part of the tile %lld) tile %lld | gemm1 %lld | to-lds %lld | ln %lld | gemm2 %lld | epilogue %lld | total %lld\n", p.n, blk,
               sh_tile_done - sh_t[0], sh_t[1] - sh_t[0], sh_t[2] - sh_t[1], sh_t[3] - sh_t[2], sh_t[4] - sh_t[3], sh_t[5] - sh_t[4], sh_t[6] - sh_t[5], sh_t[6] - sh_t[0]);
#endif
}

// ---- what is left of stage 1 in the coarse-to-fine chain once G and sigma exist (Stage1Args, hoisted form) ----
//     s = 1 + resize(coarser score) * alpha          (salience_transformer.py:139-143; x + x * up * alpha = s x)
//     k = s sigma / sqrt(s^2 sigma^2 + eps)
//     z = GELU(k G + c0):  z[:128] -> z_local,  sum over the block's tokens of z[128:] -> partial   (as stage 1 leaves them)
struct ModulateArgs {
    const float *g;            // [B, n, 256] of this level, images g_batch_stride apart
    int64_t g_batch_stride;
    const float *sigma;        // [B, n], images sigma_batch_stride apart
    int64_t sigma_batch_stride;
    const float *row_scale;    // [B, n] or NULL
    const float *coarse;       // [B, ch, cw] coarser score map or NULL
    int ch, cw, h, w;
    const float *alpha;        // device scalar (NULL = 1)
    float eps1;
    const float *c0;           // [256] W beta + b
    float *z_local;            // [B, n, 128]
    float *partial;            // [B, nblk, 128]
    int n, nblk;
    float *score_min_init;     // optional device scalar set to +inf (what the const launch does for stage 2's minimum, when
                               // stage 2 takes the constant in its own blocks and that launch does not exist)
};

constexpr int kModThreads = 256;
constexpr int kModLdsFloats = 32 + 4 * kHalf;   // k per token | the waves' column sums

// Block = 32 tokens (stage 1's blocking: `partial` has the same rows) on 256 threads: wave w takes tokens w, w + 4, ...,
// lane l channels 4l .. 4l + 3 -- a row of G is one coalesced KB, all eight in flight.  `tid` = the thread's index among
// the 256 of its block, `lds` their kModLdsFloats: a 512-thread workgroup of a launch that carries jobs runs two blocks
// (were its upper half to exit, the launch would start twice the waves for the same work: 20.4 us for the finest level
// instead of 18.4).
__device__ __forceinline__ void modulate_body(const ModulateArgs &p, int blk, int b, float *lds, int tid)
{
    constexpr int TM = 32;
    float *kk = lds, *red = lds + 32;
    const int lane = tid & 63, wave = tid >> 6;
    const int t0 = blk * TM;
    const int nvalid = min(TM, p.n - t0);
    if (p.score_min_init && blk == 0 && b == 0 && tid == 0) *p.score_min_init = INFINITY;
    // The k phase's operands are requested FIRST (sigma, the four coarse scores): loads return in order, and behind the
    // wave's eight rows of G the factor -- hence the barrier, hence every wave's GELUs -- would wait for all of them; the
    // launch then ran as three chip-wide phases (load 9 us, GELU 5, store 3) instead of one stream.
    float sg = 0.f, v00 = 0.f, v01 = 0.f, v10 = 0.f, v11 = 0.f, ly = 0.f, lx = 0.f;
    const bool modulated = p.row_scale || p.coarse;
    if (tid < TM) {
        const int t = min(t0 + tid, p.n - 1);
        sg = p.sigma[(int64_t)b * p.sigma_batch_stride + t];
        if (p.row_scale) {
            v00 = p.row_scale[(int64_t)b * p.n + t];
        } else if (p.coarse) {
            // bilinear, align_corners=True (F.interpolate, salience_transformer.py:139-142) -- as in stage1_x3_body
            const int y = t / p.w, x = t - y * p.w;
            const float sh = p.h > 1 ? (float)(p.ch - 1) / (float)(p.h - 1) : 0.f;
            const float sw = p.w > 1 ? (float)(p.cw - 1) / (float)(p.w - 1) : 0.f;
            const float fy = sh * (float)y, fx = sw * (float)x;
            const int y1 = (int)fy, x1 = (int)fx;
            const int yp = y1 < p.ch - 1 ? 1 : 0, xp = x1 < p.cw - 1 ? 1 : 0;
            ly = fy - (float)y1;
            lx = fx - (float)x1;
            const float *cm = p.coarse + (int64_t)b * p.ch * p.cw;
            v00 = cm[y1 * p.cw + x1]; v01 = cm[y1 * p.cw + x1 + xp];
            v10 = cm[(y1 + yp) * p.cw + x1]; v11 = cm[(y1 + yp) * p.cw + x1 + xp];
        }
    }
    const float *gb = p.g + (int64_t)b * p.g_batch_stride + (int64_t)t0 * kC + 4 * lane;
    float4 gv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) gv[i] = *reinterpret_cast<const float4 *>(gb + (int64_t)min(wave + 4 * i, nvalid - 1) * kC);
    const float4 c0 = *reinterpret_cast<const float4 *>(p.c0 + 4 * lane);
    if (tid < TM) {
        // s = 1 + up * alpha as an unevaluated sum s + s_lo (exact product error, TwoSum): where up * alpha comes close to
        // -1 the rounding of the plain sum (half an ulp of 1) is a RELATIVE error of 1e-5 and more in s, hence in k and in
        // every channel of the row alike -- the per-level form makes the same rounding per element, where it averages out
        float s = 1.f, s_lo = 0.f;
        if (modulated) {
            float up = v00;
            if (!p.row_scale) {
                const float hy = 1.f - ly, hx = 1.f - lx;
                up = hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11);
            }
            const float a = p.alpha ? *p.alpha : 1.f;
            const float pr = up * a, pe = fmaf(up, a, -pr);
            s = 1.f + pr;
            const float bb = s - 1.f;
            s_lo = ((1.f - (s - bb)) + (pr - bb)) + pe;
        }
        const float ss = fmaf(s_lo, sg, s * sg);
        kk[tid] = ss * rsqrtf(fmaf(ss, ss, p.eps1));
    }
    __syncthreads();
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float *zl = p.z_local + ((int64_t)b * p.n + t0) * kHalf + 4 * lane;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int r = wave + 4 * i;
        const float k = kk[r];
        const float4 z = make_float4(gelu_erf(fmaf(k, gv[i].x, c0.x)), gelu_erf(fmaf(k, gv[i].y, c0.y)),
                                     gelu_erf(fmaf(k, gv[i].z, c0.z)), gelu_erf(fmaf(k, gv[i].w, c0.w)));
        if (r < nvalid) {
            if (lane < 32) {
                *reinterpret_cast<float4 *>(zl + (int64_t)r * kHalf) = z;
            } else {
                acc.x += z.x; acc.y += z.y; acc.z += z.z; acc.w += z.w;
            }
        }
    }
    if (lane >= 32) *reinterpret_cast<float4 *>(red + wave * kHalf + 4 * (lane - 32)) = acc;
    __syncthreads();
    if (tid < kHalf)
        p.partial[((int64_t)b * p.nblk + blk) * kHalf + tid] =
            (red[tid] + red[kHalf + tid]) + (red[2 * kHalf + tid] + red[3 * kHalf + tid]);
}

struct Stage2Args {
    const float *z_local;   // [B, n, 128]
    const float *cst;       // [B, 128]
    const float4 *w2a;      // packed W2[:, :128]   (128 x 128)
    const void *w2a_x3;     // the same as three bf16 planes (sdetr_pack_linear_bf16x3) or NULL: the first product then runs on
                            // the bf16 matrix cores at fp32 accuracy like stage 1's (round 6; `w2a` is not read)
    const float4 *w3;       // packed W3            (64 x 128)
    const float *b3, *w4, *b4;
    float *score;           // [B, n]
    float *score2;          // optional second destination, row stride score2_stride (flattened score buffer)
    float *score_min;       // optional device scalar: min over every score of the launch (initialised by const kernel)
    int64_t score2_stride;
    int n;
    // The per-image constant IN the block (partial != NULL; round 6, levels of up to kConstInBlockRows rows of partial
    // sums): every block sums the level's partial sums and takes the 128 x 128 product itself -- the same numbers in every
    // block (one fixed order), and the const launch (4.6-4.9 us on the coarse levels, the chip idle) disappears.
    const float *partial = nullptr;   // [B, partial_rows, 128]
    int partial_rows = 0;
    const float *w2 = nullptr, *b2 = nullptr;   // layer2[0] weight [128, 256] / bias [128]
};

constexpr int kConstInBlockRows = 160;

// const[j] = b2[j] + sum_c W2[j][128 + c] * mean_c, mean_c = (sum over the rows of partial) / n, by the block's 256 threads
// in `scratch` (512 floats); the result is scratch[384 + j] (a barrier has been passed).
__device__ __forceinline__ void stage2_const_in_block(const float *partial, int rows, int n, const float *w2, const float *b2,
                                                      float *scratch, int tid)
{
    const int j = tid & (kHalf - 1), g = tid >> 7;   // two groups take the rows in turns, eight in flight each
    const float *pp = partial + j;
    float s[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) s[u] = 0.f;
    for (int i = g; i < rows; i += 16) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = i + 2 * u < rows ? pp[(int64_t)(i + 2 * u) * kHalf] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) s[u] += v[u];
    }
    scratch[g * kHalf + j] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
    __syncthreads();
    if (tid < kHalf) scratch[2 * kHalf + tid] = (scratch[tid] + scratch[kHalf + tid]) / (float)n;
    __syncthreads();
    const int j2 = tid >> 1, q = tid & 1;   // two threads per output row, 64 columns each
    const float *wr = w2 + (int64_t)j2 * kC + kHalf + q * 64;
    const float *mean = scratch + 2 * kHalf + q * 64;
    float a = 0.f;
#pragma unroll
    for (int c = 0; c < 64; c += 4) {
        const float4 wv = *reinterpret_cast<const float4 *>(wr + c);
        a += (wv.x * mean[c] + wv.y * mean[c + 1]) + (wv.z * mean[c + 2] + wv.w * mean[c + 3]);
    }
    a += __shfl_xor(a, 1);
    if (q == 0) scratch[3 * kHalf + j2] = b2[j2] + a;
    __syncthreads();
}

constexpr int kStage2TileFloats = kS2Planes / 4 > kTM * kZS ? kS2Planes / 4 : kTM * kZS;   // the planes of the x3 form | the fp32 tile
constexpr int kStage2LdsFloats = kStage2TileFloats + 2 * kTM;   // zt | red

// (`blk` / `b` = token block and image; `zt` [kTM * kZS] and `red` [2 * kTM] floats of LDS: the kernel's own static
// arrays, or a piece of the dynamic LDS of a launch that also carries other work -- fused_head_value.hip.  The first
// 256 threads of the workgroup take part.)
__device__ __forceinline__ void stage2_body(const Stage2Args &p, int blk, int b, float *zt, float *red)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t0 = blk * kTM;
    const int nvalid = min(kTM, p.n - t0);
#ifdef SH_STAMPS
    long long s2_t[8];
    int s2_n = 0;
#define S2_STAMP() s2_t[s2_n++] = clock64()
#else
#define S2_STAMP()
#endif
    S2_STAMP();
    const bool x3 = p.w2a_x3 != nullptr;
    WeightStream<1, 8> ws;
    WeightStreamX3G<kHalf / 32, 4> ws3;
    if (x3) ws3.start(p.w2a_x3, kHalf / 16, wave, lane);
    else ws.start(p.w2a, kHalf, kHalf / 8, wave * 32, lane);
    const int rt2 = wave >> 1, ct2 = wave & 1;
    const float bias3 = p.b3[ct2 * 32 + (lane & 31)], wo = p.w4[ct2 * 32 + (lane & 31)], b4 = p.b4[0];
    float cb;
    {
        const float *zb = p.z_local + ((int64_t)b * p.n + t0) * kHalf;
        float4 v[kTM * (kHalf / 4) / kBlock];
#pragma unroll
        for (int i = 0; i < kTM * (kHalf / 4) / kBlock; ++i) {
            const int idx = tid + i * kBlock;
            const int r = idx >> 5, c4 = idx & 31;
            v[i] = *reinterpret_cast<const float4 *>(zb + (int64_t)min(r, nvalid - 1) * kHalf + c4 * 4);
        }
        if (p.partial) {
            // (the tile's rows are on their way; the tile's LDS is the scratch until they are stored)
            stage2_const_in_block(p.partial + (int64_t)b * p.partial_rows * kHalf, p.partial_rows, p.n, p.w2, p.b2, zt, tid);
            cb = zt[3 * kHalf + wave * 32 + (lane & 31)];
            __syncthreads();
        } else {
            cb = p.cst[(int64_t)b * kHalf + wave * 32 + (lane & 31)];
        }
#pragma unroll
        for (int i = 0; i < kTM * (kHalf / 4) / kBlock; ++i) {
            const int idx = tid + i * kBlock;
            const int r = idx >> 5, c4 = idx & 31;
            const float4 val = r < nvalid ? v[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            if (x3) {   // three bf16 planes [64][128] (the fp32 tile of the second product takes their place later)
                uint2 p0, p1, p2;
                split3<false>(val, p0, p1, p2);
                char *d = reinterpret_cast<char *>(zt) + r * kS2PlaneRow + c4 * 8;
                *reinterpret_cast<uint2 *>(d) = p0;
                *reinterpret_cast<uint2 *>(d + kS2PlaneBytes) = p1;
                *reinterpret_cast<uint2 *>(d + 2 * kS2PlaneBytes) = p2;
            } else {
                *reinterpret_cast<float4 *>(zt + r * kZS + c4 * 4) = val;
            }
        }
    }
    __syncthreads();
    S2_STAMP();   // 1: tile in LDS
    // layer2[0] (local half; the global half is the per-image constant) + GELU: wave w -> columns [32w, 32w+32)
    {
        f32x16 acc[2][1];
        zero_acc(acc);
        if (x3) {
            f32x16 a3[2] = {acc[0][0], acc[1][0]};
            block_gemm_x3g<kHalf, 64, 2, kHalf / 32, 4>(reinterpret_cast<const char *>(zt), ws3, lane, a3);
            acc[0][0] = a3[0];
            acc[1][0] = a3[1];
        } else {
            block_gemm<kHalf, kZS, 2, 1, 8>(zt, ws, lane, acc);
        }
        S2_STAMP();   // 2: first product
        ws.start(p.w3, kHalf / 2, kHalf / 8, ct2 * 32, lane);
        __syncthreads();
        const int c = wave * 32 + (lane & 31);
#pragma unroll
        for (int rt = 0; rt < 2; ++rt)
#pragma unroll
            for (int i = 0; i < 16; ++i) zt[(32 * rt + acc_row(i, lane)) * kZS + c] = gelu_erf(acc[rt][0][i] + cb);
    }
    __syncthreads();
    S2_STAMP();   // 3: GELU, hidden state in LDS
    // layer2[2] + GELU, layer2[4]: wave -> (row tile, column tile) of the [64 x 64] hidden state
    {
        f32x16 acc[1][1];
        zero_acc(acc);
        block_gemm<kHalf, kZS, 1, 1, 8>(zt + rt2 * 32 * kZS, ws, lane, acc);
        S2_STAMP();   // 4: second product
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            float v = gelu_erf(acc[0][0][i] + bias3) * wo;
#ifdef SH_BUTTERFLY_LAST
            // (until round 6: the butterfly v[i] += v[i ^ o], o = 16 ... 1, five trips through the LDS crossbar per element)
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 32);
            if ((lane & 31) == 0) red[ct2 * kTM + 32 * rt2 + acc_row(i, lane)] = v;
#else
            // sum over the 32 lanes of the column tile, INTO lane 31 of the half-wave: shifts inside the rows of 16, then
            // row 0's total broadcast into row 1 -- DPP steps only, no LDS instruction (round 6; the 16 x 5 shuffles of
            // the butterfly were 4 400 of the workgroup's 22 000 cycles on an empty chip and 16 000 in the finest
            // level's launch, behind the other workgroups' fragment reads)
            v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xf, 0xf, true));   // row_shr:1
            v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x112, 0xf, 0xf, true));   // row_shr:2
            v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x114, 0xf, 0xf, true));   // row_shr:4
            v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x118, 0xf, 0xf, true));   // row_shr:8
            v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x142, 0xa, 0xf, true));   // row_bcast:15 -> rows 1, 3
            if ((lane & 31) == 31) red[ct2 * kTM + 32 * rt2 + acc_row(i, lane)] = v;
#endif
        }
    }
    __syncthreads();
    float s = INFINITY;
    if (tid < nvalid) {
        s = (red[tid] + red[kTM + tid]) + b4;
        p.score[(int64_t)b * p.n + t0 + tid] = s;
        if (p.score2) p.score2[(int64_t)b * p.score2_stride + t0 + tid] = s;
    }
    if (p.score_min && tid < kTM) {   // wave 0 holds the block's scores: min is order-independent, so atomics are exact
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s = fminf(s, __shfl_xor(s, o));
        if (tid == 0) {
            // float min through integer atomics: non-negative floats order like signed ints, negative ones reversed
            if (s >= 0.f) atomicMin(reinterpret_cast<int *>(p.score_min), __float_as_int(s));
            else atomicMax(reinterpret_cast<unsigned int *>(p.score_min), __float_as_uint(s));
        }
    }
#ifdef SH_STAMPS
    S2_STAMP();   // 5: GELU, the last layer's dot product over the 64 hidden units, scores
    if (tid == 0 && b == 0 && (blk == 0 || blk == (p.n / kTM) / 2))
        printf("stage2 n=%d blk=%d cycles: tile %lld | gemm1 %lld | gelu %lld | gemm2 %lld | last %lld | total %lld\n", p.n, blk,
               s2_t[1] - s2_t[0], s2_t[2] - s2_t[1], s2_t[3] - s2_t[2], s2_t[4] - s2_t[3], s2_t[5] - s2_t[4], s2_t[5] - s2_t[0]);
#endif
}

}  // namespace sdetr

#pragma clang fp contract(fast)

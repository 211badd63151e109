// The Swin backbone's backward (training; swin.hip is the forward).  For a block
//   u = x + s1[n] * proj(attention(qkv(LN1(x)))),  y = u + s2[n] * fc2(gelu(fc1(LN2(u))))
// and a patch merging reduction(LN(gather(y))).  The residual-stream gradient is channels-last fp32 in every precision; the
// GEMM operands, the qkv rows and their gradient are in the compute dtype.  The Linears go to backbone_backward.hip's
// backward-data / backward-weight kernels and the rows / GELU / LayerNorm / ingest kinds to convnext_backward.hip's, both
// through sdetr_convnext_bwd_op_run (nothing of them is repeated here); new are
//   swb_attention_kernel   window attention backward.  A workgroup owns one head and a strip of windows.  Per window the
//                          head's q / k / v and dO are staged in LDS as the forward stages them (padded tokens carry the
//                          bias, their dO is zero; the roll is index arithmetic).  Pass 1, a wave per 16-query tile: S^T and
//                          the two-pass softmax as the forward, dP^T = V dO^T in the same layout, D = rowsum(P dP),
//                          dS = P (dP - D) in registers, dQ^T = K^T dS^T; the row statistics (max, 1 / sum, D) go to LDS.
//                          Pass 2, a wave per 16-key tile: S and dP recomputed key-major from those statistics, 32 queries
//                          at a time, dK^T = Q^T dS and dV^T = dO^T P accumulated over the queries.  Neither S nor dS ever
//                          touches LDS.  dS (the table gradient) and the padded tokens' dK / dV (qkv bias gradient) are
//                          accumulated in registers over the strip: one partial per (strip, head)
//   swb_pad_finish / swb_table_reduce / swb_table_scatter   the partials added in strip order; the table gradient then
//                          summed over the (query, key) pairs of one table entry in the order of the CSR list
//   swb_colsum_kernel / swb_colsum_finish   column sums of compute-dtype rows (+ a vector): the qkv bias gradient
//   swb_gather_kernel / swb_scatter_kernel  patch merging: the 2 x 2 gather as fp32 rows in front of the LayerNorm
//                          backward, and its input gradient scattered back to the pixels (+ add)
// No atomics: every sum has a fixed order.  Every launch writes every element of its outputs.
#include "backbone_rows_core.h"

namespace sdetr {
namespace {

constexpr int kSbThreads = 256;
constexpr int kSbHd = 32;

typedef float sb_f32x4_t __attribute__((ext_vector_type(4)));

struct SbAttn {
    const char *qkv;      // rows [M][3 C], compute dtype
    const char *dout;     // rows [M][C], compute dtype
    const float *bias;    // [3 C]
    const float *table;   // [heads][N][N]
    char *dqkv;           // rows [M][3 C], compute dtype
    float *ptable;        // [strips][heads][N * N]
    float *ppad;          // [strips][heads][2][32]: the padded tokens' dK | dV sums
    int batch, h, w, c, ph, pw, nwx, nwy, sh, sw, heads, windows, strips;
};

template <bool F32, int WS>
struct SbCfg {
    static constexpr int kN = WS * WS;                          // 49 | 144 tokens
    static constexpr int kNK = (kN + 31) / 32 * 32;             // 64 | 160 rows: whole 32-token steps of the second products
    static constexpr int kQT = (kN + 15) / 16;                  // 4 | 9 tiles of 16 tokens that hold a token
    static constexpr int kTPW = (kQT + 3) / 4;                  // 1 | 3 query tiles per wave
    static constexpr int kRow = F32 ? (kSbHd + 4) * 4 : (kSbHd + 8) * 2;   // bytes per q / k / v / dO row: 144 | 80
    static constexpr int kTRow = (kNK + 8) * 2;                 // bytes per transposed 16-bit row: 144 | 336
    static constexpr int kQ = 0, kK = kNK * kRow, kV = 2 * kNK * kRow, kD = 3 * kNK * kRow;
    static constexpr int kKT = 4 * kNK * kRow;                  // 16-bit only: K^T, Q^T, dO^T [32][NK]
    static constexpr int kQTr = kKT + kSbHd * kTRow, kDT = kQTr + kSbHd * kTRow;
    static constexpr int kStat = F32 ? kKT : kDT + kSbHd * kTRow;   // [3][NK] f32: row max, 1 / row sum, D
    static constexpr int kIdx = kStat + 3 * kNK * 4;            // [2][NK] int: the token's row of qkv, its mask region
    static constexpr int kLds = kIdx + 2 * kNK * 4;
};

__device__ __forceinline__ sb_f32x4_t sb_mfma_f32(float a, float b, sb_f32x4_t c)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ sb_f32x4_t sb_zero() { return sb_f32x4_t{0.f, 0.f, 0.f, 0.f}; }

// c[r] += sum over the 32 channels of A[16 tile + 4 g + r][.] * B[col][.]: the row-major product both passes take
// (A rows of the tile from LDS at `arows`, B = this lane's row `brow`)
template <bool F32, int ROW>
__device__ __forceinline__ sb_f32x4_t sb_rows_product(const char *arows, const char *brow, int t16, int g)
{
    sb_f32x4_t c = sb_zero();
    if (F32) {
#pragma unroll
        for (int st = 0; st < 8; ++st)
            c = sb_mfma_f32(*reinterpret_cast<const float *>(arows + t16 * ROW + (4 * st + g) * 4),
                            *reinterpret_cast<const float *>(brow + (4 * st + g) * 4), c);
    } else {
        c = mfma_act_16x16x32(*reinterpret_cast<const uint4 *>(arows + t16 * ROW + g * 16),
                              *reinterpret_cast<const uint4 *>(brow + g * 16), c);
    }
    return c;
}

template <bool F32, int WS>
__global__ void __launch_bounds__(kSbThreads) swb_attention_kernel(SbAttn a)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    using Cfg = SbCfg<F32, WS>;
    constexpr int N = Cfg::kN, NK = Cfg::kNK, KT = NK / 16, QT = Cfg::kQT, TPW = Cfg::kTPW, ESZ = F32 ? 4 : 2;
    constexpr int ROW = Cfg::kRow, TROW = Cfg::kTRow;
    constexpr int kPieces = F32 ? 8 : 4, kPer = F32 ? 4 : 8;    // 16-byte pieces per 32-wide head slice, values per piece
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t16 = lane & 15, g = lane >> 4;
    const int head = blockIdx.y, strip = blockIdx.x;
    const int per_img = a.nwx * a.nwy;
    float *stat_m = reinterpret_cast<float *>(lds + Cfg::kStat), *stat_l = stat_m + NK, *stat_d = stat_l + NK;
    int *rowi = reinterpret_cast<int *>(lds + Cfg::kIdx);       // [NK]: the token's row of qkv, -1 = a token of the padding
    int *region = rowi + NK;                                    // [NK]: 3 * row region + column region
    const bool masked = a.sh > 0 || a.sw > 0;                   // (uniform)
    const float scale = 0.17677669529663687f;                   // 32^-0.5

    sb_f32x4_t tacc[TPW][KT];                                   // dS of this wave's query tiles, summed over the strip
#pragma unroll
    for (int i = 0; i < TPW; ++i)
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) tacc[i][kt] = sb_zero();
    sb_f32x4_t pacc[2][2] = {{sb_zero(), sb_zero()}, {sb_zero(), sb_zero()}};   // [dK | dV][dt] of padded keys (lane t16's)

    for (int win = strip; win < a.windows; win += a.strips) {
        const int n = win / per_img, wi = win - n * per_img;
        const int wy = wi / a.nwx, wx = wi - wy * a.nwx;
        __syncthreads();                                        // the previous window's readers are done
        for (int t = tid; t < NK; t += kSbThreads) {
            int ri = -2, rg = 0;
            if (t < N) {
                const int ty = t / WS, tx = t - ty * WS;
                const int cy = wy * WS + ty, cx = wx * WS + tx; // in the rolled frame
                int py = cy + a.sh, px = cx + a.sw;             // in the padded map
                if (py >= a.ph) py -= a.ph;
                if (px >= a.pw) px -= a.pw;
                ri = (py < a.h && px < a.w) ? (n * a.h + py) * a.w + px : -1;
                const int ry = a.sh > 0 ? (cy < a.ph - WS ? 0 : (cy < a.ph - a.sh ? 1 : 2)) : 0;
                const int rx = a.sw > 0 ? (cx < a.pw - WS ? 0 : (cx < a.pw - a.sw ? 1 : 2)) : 0;
                rg = 3 * ry + rx;
            }
            rowi[t] = ri;
            region[t] = rg;
        }
        __syncthreads();

        // q | k | v | dO of this head, 16 bytes per item; a padded token carries the bias and a zero dO, a row past N zeros
        for (int i = tid; i < NK * 4 * kPieces; i += kSbThreads) {
            const int t = i / (4 * kPieces), rem = i - t * 4 * kPieces, part = rem / kPieces, piece = rem - part * kPieces;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (t < N) {
                const int ri = rowi[t];
                if (part == 3) {
                    if (ri >= 0) v = *reinterpret_cast<const uint4 *>(a.dout + ((int64_t)ri * a.c + head * kSbHd + piece * kPer) * ESZ);
                } else {
                    const int col = part * a.c + head * kSbHd + piece * kPer;
                    if (ri >= 0) {
                        v = *reinterpret_cast<const uint4 *>(a.qkv + ((int64_t)ri * 3 * a.c + col) * ESZ);
                    } else if (F32) {
                        v = *reinterpret_cast<const uint4 *>(a.bias + col);
                    } else {
                        const float4 b0 = *reinterpret_cast<const float4 *>(a.bias + col), b1 = *reinterpret_cast<const float4 *>(a.bias + col + 4);
                        v = make_uint4(pack_act2(b0.x, b0.y), pack_act2(b0.z, b0.w), pack_act2(b1.x, b1.y), pack_act2(b1.z, b1.w));
                    }
                }
            }
            *reinterpret_cast<uint4 *>(lds + part * NK * ROW + t * ROW + piece * 16) = v;
            if (!F32 && part != 2) {                            // K^T, Q^T, dO^T [32][NK] for the second products
                uint16_t *tr = reinterpret_cast<uint16_t *>(lds + (part == 1 ? Cfg::kKT : (part == 0 ? Cfg::kQTr : Cfg::kDT)));
                const uint32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    tr[(piece * 8 + 2 * j) * (TROW / 2) + t] = (uint16_t)(e[j] & 0xffffu);
                    tr[(piece * 8 + 2 * j + 1) * (TROW / 2) + t] = (uint16_t)(e[j] >> 16);
                }
            }
        }
        __syncthreads();

        // ---- pass 1: a wave per 16-query tile; lane (t16, g) holds query qi and keys 16 kt + 4 g + r
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            const int qt = wave + 4 * i;
            if (qt >= QT) break;                                // (uniform)
            const int qi = 16 * qt + t16;
            const char *qrow = lds + Cfg::kQ + qi * ROW, *drow = lds + Cfg::kD + qi * ROW;
            sb_f32x4_t s[KT], dp[KT];
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                s[kt] = sb_rows_product<F32, ROW>(lds + Cfg::kK + 16 * kt * ROW, qrow, t16, g);
                dp[kt] = sb_rows_product<F32, ROW>(lds + Cfg::kV + 16 * kt * ROW, drow, t16, g);
            }
            const int qc = min(qi, N - 1);                      // (a query row past N has dO = 0: its dS is zero)
            const float *tb = a.table + ((int64_t)head * N + qc) * N;
            const int qreg = region[qc];
            float mx = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int kj = 16 * kt + 4 * g + r;
                    float v = -INFINITY;
                    if (kj < N) {
                        v = fmaf(s[kt][r], scale, tb[kj]);
                        if (masked && region[kj] != qreg) v -= 100.f;
                    }
                    s[kt][r] = v;
                    mx = fmaxf(mx, v);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 16));
            mx = fmaxf(mx, __shfl_xor(mx, 32));
            float sum = 0.f;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = expf(s[kt][r] - mx);
                    s[kt][r] = p;
                    sum += p;
                }
            sum += __shfl_xor(sum, 16);
            sum += __shfl_xor(sum, 32);
            const float inv = 1.f / sum;
            float dsum = 0.f;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[kt][r] *= inv;
                    dsum = fmaf(s[kt][r], dp[kt][r], dsum);
                }
            dsum += __shfl_xor(dsum, 16);
            dsum += __shfl_xor(dsum, 32);
            if (g == 0) {
                stat_m[qi] = mx;
                stat_l[qi] = inv;
                stat_d[qi] = dsum;
            }
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    s[kt][r] *= dp[kt][r] - dsum;               // dS
                    tacc[i][kt][r] += s[kt][r];
                }
            // dQ^T = K^T dS^T: o[dt][r] = channel 16 dt + 4 g + r of query qi
            sb_f32x4_t o[2] = {sb_zero(), sb_zero()};
            if (F32) {
#pragma unroll
                for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const char *krow = lds + Cfg::kK + (16 * kt + 4 * g + r) * ROW;
#pragma unroll
                        for (int dt = 0; dt < 2; ++dt)
                            o[dt] = sb_mfma_f32(*reinterpret_cast<const float *>(krow + (16 * dt + t16) * 4), s[kt][r], o[dt]);
                    }
            } else {
#pragma unroll
                for (int u = 0; u < KT / 2; ++u) {               // lane group g holds keys {4g .. 4g+3, 16+4g .. 16+4g+3} of a 32-key block
                    const uint4 pf = make_uint4(pack_act2(s[2 * u][0], s[2 * u][1]), pack_act2(s[2 * u][2], s[2 * u][3]),
                                                pack_act2(s[2 * u + 1][0], s[2 * u + 1][1]), pack_act2(s[2 * u + 1][2], s[2 * u + 1][3]));
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) {
                        const char *kt_row = lds + Cfg::kKT + (16 * dt + t16) * TROW + (32 * u + 4 * g) * 2;
                        const uint2 lo = *reinterpret_cast<const uint2 *>(kt_row), hi = *reinterpret_cast<const uint2 *>(kt_row + 32);
                        o[dt] = mfma_act_16x16x32(make_uint4(lo.x, lo.y, hi.x, hi.y), pf, o[dt]);
                    }
                }
            }
            const int ri = qi < N ? rowi[qi] : -2;
            if (ri >= 0) {                                       // (a padded token's dQ is zero: its output row was dropped)
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    char *dst = a.dqkv + ((int64_t)ri * 3 * a.c + head * kSbHd + 16 * dt + 4 * g) * ESZ;
                    const float v0 = o[dt][0] * scale, v1 = o[dt][1] * scale, v2 = o[dt][2] * scale, v3 = o[dt][3] * scale;
                    if (F32) *reinterpret_cast<float4 *>(dst) = make_float4(v0, v1, v2, v3);
                    else *reinterpret_cast<uint2 *>(dst) = make_uint2(pack_act2(v0, v1), pack_act2(v2, v3));
                }
            }
        }
        __syncthreads();                                         // the row statistics are in LDS

        // ---- pass 2: a wave per 16-key tile; lane (t16, g) holds key kj and queries 16 qt + 4 g + r
        for (int kt = wave; kt < QT; kt += kSbThreads / 64) {
            const int kj = 16 * kt + t16;
            const bool kvalid = kj < N;
            const int kc = min(kj, N - 1), kreg = region[kc];
            const char *krow = lds + Cfg::kK + kj * ROW, *vrow = lds + Cfg::kV + kj * ROW;
            const float *tb = a.table + (int64_t)head * N * N + kc;
            sb_f32x4_t ok[2] = {sb_zero(), sb_zero()}, ov[2] = {sb_zero(), sb_zero()};
#pragma unroll 1
            for (int u = 0; u < KT / 2; ++u) {
                sb_f32x4_t p[2], ds[2];
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    const int qt = 2 * u + hf;
                    const sb_f32x4_t st = sb_rows_product<F32, ROW>(lds + Cfg::kQ + 16 * qt * ROW, krow, t16, g);
                    const sb_f32x4_t dpt = sb_rows_product<F32, ROW>(lds + Cfg::kD + 16 * qt * ROW, vrow, t16, g);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int q = 16 * qt + 4 * g + r;
                        float pv = 0.f, dv = 0.f;
                        if (kvalid && q < N) {
                            float v = fmaf(st[r], scale, tb[(int64_t)q * N]);
                            if (masked && region[q] != kreg) v -= 100.f;
                            pv = expf(v - stat_m[q]) * stat_l[q];
                            dv = pv * (dpt[r] - stat_d[q]);
                        }
                        p[hf][r] = pv;
                        ds[hf][r] = dv;
                    }
                }
                // dV^T += dO^T P, dK^T += Q^T dS over these 32 queries
                if (F32) {
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int q = 16 * (2 * u + hf) + 4 * g + r;
                            const char *qrow = lds + Cfg::kQ + q * ROW, *drow = lds + Cfg::kD + q * ROW;
#pragma unroll
                            for (int dt = 0; dt < 2; ++dt) {
                                ov[dt] = sb_mfma_f32(*reinterpret_cast<const float *>(drow + (16 * dt + t16) * 4), p[hf][r], ov[dt]);
                                ok[dt] = sb_mfma_f32(*reinterpret_cast<const float *>(qrow + (16 * dt + t16) * 4), ds[hf][r], ok[dt]);
                            }
                        }
                } else {
                    const uint4 pf = make_uint4(pack_act2(p[0][0], p[0][1]), pack_act2(p[0][2], p[0][3]), pack_act2(p[1][0], p[1][1]),
                                                pack_act2(p[1][2], p[1][3]));
                    const uint4 df = make_uint4(pack_act2(ds[0][0], ds[0][1]), pack_act2(ds[0][2], ds[0][3]),
                                                pack_act2(ds[1][0], ds[1][1]), pack_act2(ds[1][2], ds[1][3]));
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt) {
                        const int off = (16 * dt + t16) * TROW + (32 * u + 4 * g) * 2;
                        const uint2 dl = *reinterpret_cast<const uint2 *>(lds + Cfg::kDT + off);
                        const uint2 dh = *reinterpret_cast<const uint2 *>(lds + Cfg::kDT + off + 32);
                        ov[dt] = mfma_act_16x16x32(make_uint4(dl.x, dl.y, dh.x, dh.y), pf, ov[dt]);
                        const uint2 ql = *reinterpret_cast<const uint2 *>(lds + Cfg::kQTr + off);
                        const uint2 qh = *reinterpret_cast<const uint2 *>(lds + Cfg::kQTr + off + 32);
                        ok[dt] = mfma_act_16x16x32(make_uint4(ql.x, ql.y, qh.x, qh.y), df, ok[dt]);
                    }
                }
            }
            const int ri = kvalid ? rowi[kj] : -2;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const float k0 = ok[dt][0] * scale, k1 = ok[dt][1] * scale, k2 = ok[dt][2] * scale, k3 = ok[dt][3] * scale;
                if (ri >= 0) {
                    char *dk = a.dqkv + ((int64_t)ri * 3 * a.c + a.c + head * kSbHd + 16 * dt + 4 * g) * ESZ;
                    char *dv = dk + (int64_t)a.c * ESZ;
                    if (F32) {
                        *reinterpret_cast<float4 *>(dk) = make_float4(k0, k1, k2, k3);
                        *reinterpret_cast<float4 *>(dv) = make_float4(ov[dt][0], ov[dt][1], ov[dt][2], ov[dt][3]);
                    } else {
                        *reinterpret_cast<uint2 *>(dk) = make_uint2(pack_act2(k0, k1), pack_act2(k2, k3));
                        *reinterpret_cast<uint2 *>(dv) = make_uint2(pack_act2(ov[dt][0], ov[dt][1]), pack_act2(ov[dt][2], ov[dt][3]));
                    }
                } else if (ri == -1) {                           // a padded key: gradient of the qkv bias
                    pacc[0][dt][0] += k0, pacc[0][dt][1] += k1, pacc[0][dt][2] += k2, pacc[0][dt][3] += k3;
                    pacc[1][dt][0] += ov[dt][0], pacc[1][dt][1] += ov[dt][1], pacc[1][dt][2] += ov[dt][2], pacc[1][dt][3] += ov[dt][3];
                }
            }
        }
    }

    // ---- the strip's partials: dS per (query, key), the padded sums per channel (lanes, then waves, in a fixed order)
    float *pt = a.ptable + ((int64_t)strip * a.heads + head) * N * N;
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int qi = 16 * (wave + 4 * i) + t16;
        if (wave + 4 * i >= QT || qi >= N) continue;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int kj = 16 * kt + 4 * g + r;
                if (kj < N) pt[qi * N + kj] = tacc[i][kt][r];
            }
    }
    __syncthreads();
    float *red = reinterpret_cast<float *>(lds);                 // [4 waves][64]
#pragma unroll
    for (int part = 0; part < 2; ++part)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = pacc[part][dt][r];
                v += __shfl_xor(v, 1);
                v += __shfl_xor(v, 2);
                v += __shfl_xor(v, 4);
                v += __shfl_xor(v, 8);
                if (t16 == 0) red[wave * 64 + part * 32 + 16 * dt + 4 * g + r] = v;
            }
    __syncthreads();
    if (tid < 64)
        a.ppad[((int64_t)strip * a.heads + head) * 64 + tid] = ((red[tid] + red[64 + tid]) + red[128 + tid]) + red[192 + tid];
}

// dbias [3 C]: zeros in the q third; else the strips' padded sums in strip order
__global__ void __launch_bounds__(256) swb_pad_finish_kernel(const float *ppad, int strips, int heads, int c, float *dbias)
{
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= 3 * c) return;
    const int part = col / c, ch = col - part * c;
    float v = 0.f;
    if (part > 0) {
        const int head = ch / kSbHd, d = ch - head * kSbHd;
        for (int s = 0; s < strips; ++s) v += ppad[((int64_t)s * heads + head) * 64 + (part - 1) * 32 + d];
    }
    dbias[col] = v;
}

// tsum [heads * N * N] = the strips' dS partials in strip order
__global__ void __launch_bounds__(256) swb_table_reduce_kernel(const float *ptable, int strips, int64_t total, float *tsum)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    float v = ptable[i];
    for (int s = 1; s < strips; ++s) v += ptable[(int64_t)s * total + i];
    tsum[i] = v;
}

// dtable [entries][heads]: the pairs of an entry in the order of the CSR list
__global__ void __launch_bounds__(256) swb_table_scatter_kernel(const float *tsum, const int *order, const int *offsets, int entries,
                                                                int heads, int nn, float *dtable)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= entries * heads) return;
    const int e = i / heads, head = i - e * heads;
    const int lo = max(0, min(offsets[e], nn)), hi = max(lo, min(offsets[e + 1], nn));
    float v = 0.f;
    for (int j = lo; j < hi; ++j) {
        const int p = order[j];
        if (p >= 0 && p < nn) v += tsum[(int64_t)head * nn + p];
    }
    dtable[i] = v;
}

// partial [strips][cols]: the column sums of a strip of rows (compute dtype); grid (column chunks, strips)
template <bool X3>
__global__ void __launch_bounds__(256) swb_colsum_kernel(const char *rows, int64_t n_rows, int cols, float *partial)
{
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= cols) return;
    float v = 0.f;
    for (int64_t r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const int64_t e = r * cols + col;
        v += X3 ? reinterpret_cast<const float *>(rows)[e] : act_lo(reinterpret_cast<const uint16_t *>(rows)[e]);
    }
    partial[(int64_t)blockIdx.y * cols + col] = v;
}

__global__ void __launch_bounds__(256) swb_colsum_finish_kernel(const float *partial, int strips, int cols, const float *add, float *out)
{
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= cols) return;
    float v = partial[col];
    for (int s = 1; s < strips; ++s) v += partial[(int64_t)s * cols + col];
    if (add) v += add[col];
    out[col] = v;
}

// x f32 [B][H][W][C] -> out f32 [B][Ho][Wo][4 C], the forward's 2 x 2 gather (row parity first), zeros past an odd H / W
__global__ void __launch_bounds__(256) swb_gather_kernel(const float *x, int batch, int h, int w, int c, float *out)
{
    const int cq = c >> 2, ho = (h + 1) >> 1, wo = (w + 1) >> 1;
    const int64_t total = (int64_t)batch * ho * wo * c, stride = (int64_t)gridDim.x * 256;   // quads of the output
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int q = (int)(i % c);
        const int64_t r = i / c;
        const int ox = (int)(r % wo), oy = (int)((r / wo) % ho), n = (int)(r / ((int64_t)wo * ho));
        const int part = q / cq, iy = 2 * oy + (part & 1), ix = 2 * ox + (part >> 1);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (iy < h && ix < w) v = *reinterpret_cast<const float4 *>(x + (((int64_t)n * h + iy) * w + ix) * c + 4 * (q - part * cq));
        *reinterpret_cast<float4 *>(out + i * 4) = v;
    }
}

// d f32 [B][Ho][Wo][4 C] -> out f32 [B][H][W][C] (+ add): every pixel reads its own quarter of one gathered row
__global__ void __launch_bounds__(256) swb_scatter_kernel(const float *d, const float *add, int batch, int h, int w, int c, float *out)
{
    const int cq = c >> 2, ho = (h + 1) >> 1, wo = (w + 1) >> 1;
    const int64_t total = (int64_t)batch * h * w * cq, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int q = (int)(i % cq);
        const int64_t r = i / cq;
        const int px = (int)(r % w), py = (int)((r / w) % h), n = (int)(r / ((int64_t)w * h));
        const int part = (py & 1) + 2 * (px & 1);
        float4 v = *reinterpret_cast<const float4 *>(d + ((((int64_t)n * ho + (py >> 1)) * wo + (px >> 1)) * 4 + part) * c + 4 * q);
        if (add) {
            const float4 b = *reinterpret_cast<const float4 *>(add + i * 4);
            v.x += b.x, v.y += b.y, v.z += b.z, v.w += b.w;
        }
        *reinterpret_cast<float4 *>(out + i * 4) = v;
    }
}

// ------------------------------------------------------------------------------------------------------------ host
const char *kind_name(int kind)
{
    static const char *names[] = {"dgrad", "wgrad", "rows", "gelu", "layer norm", "ingest", "window attention", "column sums",
                                  "patch merging"};
    return kind >= 0 && kind <= 8 ? names[kind] : "?";
}

// kinds 0 .. 5 as the ConvNeXt backward's op (kind 5 is its ingest, 10)
sdetr_convnext_bwd_op rows_op(const sdetr_swin_bwd_op &o)
{
    sdetr_convnext_bwd_op b = {};
    b.kind = o.kind == 5 ? 10 : o.kind;
    b.dz = o.dz;
    b.x = o.x;
    b.weight = o.weight;
    b.scale = o.scale;
    b.gamma = o.gamma;
    b.add = o.add;
    b.out = o.out;
    b.dbias = o.dbias;
    b.dgamma = o.dgamma;
    b.dbeta = o.dbeta;
    b.batch = o.batch;
    b.channels = o.channels;
    b.height = o.height;
    b.width = o.width;
    b.out_channels = o.out_channels;
    b.splits = o.splits;
    b.eps = o.eps;
    return b;
}

inline int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

struct SbPlan {
    SbAttn attn;
    int strips, entries;
    int64_t rows, need;
    int64_t off_pad, off_sum;       // attention: the workspace pieces after the table partials
    int64_t off_dx, off_ln;         // merging: after the gathered rows
    sdetr_convnext_bwd_op ln;       // merging: the LayerNorm backward over the gathered rows
};

int strips_for(int requested, int64_t most, int automatic)
{
    const int64_t want = requested > 0 ? requested : automatic;
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, most));
}

int check_attention(const sdetr_swin_bwd_op &o, int precision, SbPlan &p)
{
    const char *what = "sdetr_swin_bwd (window attention)";
    if (int rc = check_rows_shape(what, o.batch, o.height, o.width, o.channels, precision)) return rc;
    if (o.splits < 0) return fail("%s: bad splits %d", what, o.splits);
    if (o.window != 7 && o.window != 12) return fail("%s: window must be 7 or 12 (got %d)", what, o.window);
    if (o.heads < 1 || o.heads > 65535 || (int64_t)o.heads * kSbHd != o.channels)
        return fail("%s: the head dimension must be %d (got %d channels over %d heads)", what, kSbHd, o.channels, o.heads);
    if (o.shift < 0 || o.shift >= o.window) return fail("%s: shift must lie in [0, window) (got %d)", what, o.shift);
    if (!o.x || !o.dz || !o.bias || !o.table || !o.out || !o.dbias) return fail("%s: null tensor", what);
    if (o.dtable && (!o.order || !o.offsets)) return fail("%s: null tensor (dtable needs order and offsets)", what);
    if (o.out == o.x || o.out == o.dz) return fail("%s: out must not alias x / dz", what);
    if (!all_aligned16(o.x, o.dz, o.bias, o.table, o.out, o.dbias, o.dtable, o.order, o.offsets))
        return fail("%s: tensors must be 16-byte aligned", what);
    SbAttn &a = p.attn;
    a.qkv = reinterpret_cast<const char *>(o.x);
    a.dout = reinterpret_cast<const char *>(o.dz);
    a.bias = o.bias;
    a.table = o.table;
    a.dqkv = reinterpret_cast<char *>(o.out);
    a.batch = o.batch;
    a.h = o.height;
    a.w = o.width;
    a.c = o.channels;
    a.heads = o.heads;
    a.nwy = (o.height + o.window - 1) / o.window;
    a.nwx = (o.width + o.window - 1) / o.window;
    a.ph = a.nwy * o.window;
    a.pw = a.nwx * o.window;
    a.sh = o.window >= a.ph ? 0 : o.shift;      // per axis: no shift where one window spans the padded map
    a.sw = o.window >= a.pw ? 0 : o.shift;
    const int64_t windows = (int64_t)o.batch * a.nwx * a.nwy;
    if (windows >= (int64_t(1) << 31)) return fail("%s: too many windows", what);
    a.windows = (int)windows;
    const int nn = o.window * o.window * o.window * o.window;
    // enough workgroups to fill the device twice over, fewer strips for the larger window (its partial is 83 KB)
    a.strips = strips_for(o.splits, windows, std::max(1, (o.window == 7 ? 1024 : 512) / o.heads));
    p.strips = a.strips;
    p.entries = (2 * o.window - 1) * (2 * o.window - 1);
    p.off_pad = align256((int64_t)a.strips * o.heads * nn * 4);
    p.off_sum = p.off_pad + align256((int64_t)a.strips * o.heads * 64 * 4);
    p.need = p.off_sum + align256((int64_t)o.heads * nn * 4);
    return 0;
}

int check_merge(const sdetr_swin_bwd_op &o, int precision, SbPlan &p)
{
    const char *what = "sdetr_swin_bwd (patch merging)";
    if (int rc = check_rows_shape(what, o.batch, o.height, o.width, 4 * o.channels, precision)) return rc;
    if (o.channels < 1 || (4 * o.channels) % 32 || 4 * o.channels > kRowMaxC)
        return fail("%s: 4 C must be a multiple of 32 up to %d (got C = %d)", what, kRowMaxC, o.channels);
    if (!o.dz || !o.x || !o.gamma || !o.out || (!o.dgamma != !o.dbeta)) return fail("%s: null tensor", what);
    if (!all_aligned16(o.dz, o.x, o.gamma, o.add, o.out, o.dgamma, o.dbeta)) return fail("%s: tensors must be 16-byte aligned", what);
    const int ho = (o.height + 1) / 2, wo = (o.width + 1) / 2;
    const int64_t gathered = align256((int64_t)o.batch * ho * wo * 4 * o.channels * 4);
    p.off_dx = gathered;
    p.off_ln = 2 * gathered;
    sdetr_convnext_bwd_op &b = p.ln;
    b = sdetr_convnext_bwd_op{};
    b.kind = 4;
    b.dz = o.dz;
    b.x = o.x;                      // (stands in for the gathered rows until the workspace is known: never read before)
    b.gamma = o.gamma;
    b.out = o.out;
    b.dgamma = o.dgamma;
    b.dbeta = o.dbeta;
    b.batch = o.batch;
    b.channels = 4 * o.channels;
    b.height = ho;
    b.width = wo;
    b.splits = o.splits;
    b.eps = o.eps;
    const int64_t ln = sdetr_convnext_bwd_workspace_bytes(&b, 1, precision);
    if (ln < 0) return SDETR_EINVAL;
    p.need = p.off_ln + align256(ln);
    return 0;
}

// validation of one op without a launch
int check_op(const sdetr_swin_bwd_op &o, int precision, SbPlan &p)
{
    p = SbPlan{};
    if (o.kind < 0 || o.kind > 8) return fail("sdetr_swin_bwd: unknown op kind %d", o.kind);
    if (precision != 0 && precision != 1) return fail("sdetr_swin_bwd (%s): precision must be 0 or 1", kind_name(o.kind));
    if (o.kind <= 5) {
        const sdetr_convnext_bwd_op b = rows_op(o);
        p.need = sdetr_convnext_bwd_workspace_bytes(&b, 1, precision);
        return p.need < 0 ? SDETR_EINVAL : 0;
    }
    if (o.kind == 6) return check_attention(o, precision, p);
    if (o.kind == 8) return check_merge(o, precision, p);
    const char *what = "sdetr_swin_bwd (column sums)";
    if (int rc = check_rows_shape(what, o.batch, o.height, o.width, o.channels, precision)) return rc;
    if (o.splits < 0) return fail("%s: bad splits %d", what, o.splits);
    if (!o.dz || !o.dbias) return fail("%s: null tensor", what);
    if (!all_aligned16(o.dz, o.dbias, o.add)) return fail("%s: tensors must be 16-byte aligned", what);
    p.rows = (int64_t)o.batch * o.height * o.width;
    p.strips = strips_for(o.splits, p.rows, 256);
    p.need = (int64_t)p.strips * o.channels * 4;
    return 0;
}

int check_bwd_op(const sdetr_swin_bwd_op &o, int precision, int64_t &need)
{
    SbPlan p;
    const int rc = check_op(o, precision, p);
    need = rc ? 0 : p.need;
    return rc;
}

template <bool F32, int WS>
void launch_attention(hipStream_t s, const SbAttn &a)
{
    static DeviceOnce once;
    // LDS per workgroup, 16-bit | fp32: 35 584 | 38 144 (window 7: four workgroups per CU), 86 656 | 95 360 (window 12: one)
    constexpr int bytes = SbCfg<F32, WS>::kLds;
    static_assert(bytes <= 160 * 1024, "the window attention backward fits a CU's LDS");
    allow_dynamic_lds(swb_attention_kernel<F32, WS>, once, bytes);
    hipLaunchKernelGGL((swb_attention_kernel<F32, WS>), dim3((unsigned)a.strips, (unsigned)a.heads), dim3(kSbThreads), bytes, s, a);
}

int run_bwd_op(hipStream_t s, const sdetr_swin_bwd_op &o, int precision, void *ws, int64_t ws_bytes)
{
    SbPlan p;
    if (int rc = check_op(o, precision, p)) return rc;
    const char *name = kind_name(o.kind);
    if (p.need > ws_bytes || (p.need && !ws))
        return fail("sdetr_swin_bwd (%s): workspace of %lld bytes is too small (%lld needed)", name, (long long)ws_bytes,
                    (long long)p.need);
    char *w = reinterpret_cast<char *>(ws);
    if (o.kind <= 5) {
        const sdetr_convnext_bwd_op b = rows_op(o);
        return sdetr_convnext_bwd_op_run((sdetr_stream_t)s, &b, precision, ws, ws_bytes);
    }
    if (o.kind == 6) {
        SbAttn a = p.attn;
        a.ptable = reinterpret_cast<float *>(w);
        a.ppad = reinterpret_cast<float *>(w + p.off_pad);
        float *tsum = reinterpret_cast<float *>(w + p.off_sum);
        if (precision == 0 && o.window == 7) launch_attention<true, 7>(s, a);
        else if (precision == 0) launch_attention<true, 12>(s, a);
        else if (o.window == 7) launch_attention<false, 7>(s, a);
        else launch_attention<false, 12>(s, a);
        hipLaunchKernelGGL(swb_pad_finish_kernel, dim3((unsigned)((3 * a.c + 255) / 256)), dim3(256), 0, s, a.ppad, a.strips, a.heads,
                           a.c, o.dbias);
        if (o.dtable) {
            const int nn = o.window * o.window * o.window * o.window;
            const int64_t total = (int64_t)a.heads * nn;
            hipLaunchKernelGGL(swb_table_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a.ptable, a.strips, total,
                               tsum);
            hipLaunchKernelGGL(swb_table_scatter_kernel, dim3((unsigned)((p.entries * a.heads + 255) / 256)), dim3(256), 0, s, tsum,
                               o.order, o.offsets, p.entries, a.heads, nn, o.dtable);
        }
    } else if (o.kind == 7) {
        const dim3 grid((unsigned)((o.channels + 255) / 256), (unsigned)p.strips);
        float *partial = reinterpret_cast<float *>(w);
        if (precision == 0)
            hipLaunchKernelGGL(swb_colsum_kernel<true>, grid, dim3(256), 0, s, reinterpret_cast<const char *>(o.dz), p.rows, o.channels,
                               partial);
        else
            hipLaunchKernelGGL(swb_colsum_kernel<false>, grid, dim3(256), 0, s, reinterpret_cast<const char *>(o.dz), p.rows, o.channels,
                               partial);
        hipLaunchKernelGGL(swb_colsum_finish_kernel, dim3(grid.x), dim3(256), 0, s, partial, p.strips, o.channels, o.add, o.dbias);
    } else {
        float *gathered = reinterpret_cast<float *>(w), *dx = reinterpret_cast<float *>(w + p.off_dx);
        const int ho = (o.height + 1) / 2, wo = (o.width + 1) / 2;
        const int64_t quads = (int64_t)o.batch * ho * wo * o.channels;
        hipLaunchKernelGGL(swb_gather_kernel, dim3((unsigned)std::min<int64_t>((quads + 255) / 256, 8192)), dim3(256), 0, s,
                           reinterpret_cast<const float *>(o.x), o.batch, o.height, o.width, o.channels, gathered);
        if (int rc = check_launch("sdetr_swin_bwd (patch merging)")) return rc;
        sdetr_convnext_bwd_op b = p.ln;
        b.x = gathered;
        b.out = dx;
        if (int rc = sdetr_convnext_bwd_op_run((sdetr_stream_t)s, &b, precision, w + p.off_ln, ws_bytes - p.off_ln)) return rc;
        const int64_t pix = (int64_t)o.batch * o.height * o.width * (o.channels / 4);
        hipLaunchKernelGGL(swb_scatter_kernel, dim3((unsigned)std::min<int64_t>((pix + 255) / 256, 8192)), dim3(256), 0, s, dx, o.add,
                           o.batch, o.height, o.width, o.channels, reinterpret_cast<float *>(o.out));
    }
    return check_launch("sdetr_swin_bwd");
}

}  // namespace
}  // namespace sdetr

using namespace sdetr;

using SwinBwdPlan = Plan<sdetr_swin_bwd_op, check_bwd_op, run_bwd_op>;

extern "C" int64_t sdetr_swin_bwd_workspace_bytes(const sdetr_swin_bwd_op *ops, int n_ops, int precision)
{
    return SwinBwdPlan::workspace_bytes(ops, n_ops, precision);
}

extern "C" int sdetr_swin_bwd_op_run(sdetr_stream_t stream, const sdetr_swin_bwd_op *op, int precision, void *workspace,
                                     int64_t workspace_bytes)
{
    return SwinBwdPlan::op_run("sdetr_swin_bwd", stream, op, precision, workspace, workspace_bytes);
}

extern "C" int sdetr_swin_bwd_run(sdetr_stream_t stream, const sdetr_swin_bwd_op *ops, int n_ops, int precision, void *workspace,
                                  int64_t workspace_bytes)
{
    return SwinBwdPlan::run("sdetr_swin_bwd", stream, ops, n_ops, precision, workspace, workspace_bytes);
}

// The Swin backbone, V1 (reference models/backbones/swin.py), eval mode.  As in convnext.hip / focalnet.hip the residual
// stream is channels-last fp32 [B, H, W, C] in every precision and the "compute dtype" (fp32, or the library's 16-bit type)
// is the type of the rows written between launches: the GEMM A operands, the qkv rows and the attention rows.
//
//   the GEMMs                 backbone_conv_core.h's implicit-GEMM kernel: proj / fc2 / the merging reduction / the 4x4
//                             stem on the NCHW canvas (EPI 2, fp32 stream, + residual, + NCHW copy), fc1 + GELU (EPI 1),
//                             qkv (EPI 5: acc + b in the compute dtype)
//   ln_rows_kernel            LayerNorm over C of fp32 rows, one wave per row, the row in registers (backbone_rows_core.h's)
//   swin_attention_kernel     one workgroup per (window, head): the window's q / k / v of that head staged in LDS (tokens of
//                             the zero padding synthesised from the qkv bias, the roll as index arithmetic), S^T = K Q^T
//                             per 16-query tile with all of a query's scores in registers, two-pass softmax in fp32, the
//                             scores as the B operand of O^T = V^T P^T.  16-bit: v_mfma_f32_16x16x32 (the head dimension is
//                             ONE k-step); fp32: v_mfma_f32_16x16x4_f32 on fp32 operands -- S never touches LDS
//   swin_merge_ln_kernel      the 2 x 2 gather of a patch merging + LayerNorm over 4 C, one wave per output row (its own
//                             gather, the shared row statistics and write)
// A training forward (swin_backward.hip is its backward) sets `aux` / `row_scale`: fc1 also stores its values before the GELU
// (EPI 6), proj / fc2 multiply by the branch's stochastic-depth factor per sample before the residual (EPI 7).
// The row LayerNorm, the host checks of a rows op and the plan entry points are backbone_rows_core.h's.
// No atomics; every launch writes every element of its outputs.
#include "backbone_rows_core.h"

namespace sdetr {
namespace {

constexpr int kSwThreads = 256;
constexpr int kSwHd = 32;                     // the head dimension of every V1 arch

typedef float sw_f32x4_t __attribute__((ext_vector_type(4)));

// x fp32 [B][H][W][C] -> out [B][Ho][Wo][4 C], row (i, j) = LN([x(2i, 2j) | x(2i + 1, 2j) | x(2i, 2j + 1) | x(2i + 1, 2j + 1)]):
// the row parity varies first; pixels past an odd H / W are zeros inside the statistics
template <bool F32OUT>
__global__ void __launch_bounds__(kSwThreads) swin_merge_ln_kernel(const float *x, const float *gamma, const float *beta, int batch,
                                                                   int h, int w, int c, float eps, char *out)
{
    const int lane = threadIdx.x & 63, cq = c >> 2, nq = c;          // 4 C / 4 quads per output row
    const int ho = (h + 1) >> 1, wo = (w + 1) >> 1;
    const int64_t rows = (int64_t)batch * ho * wo, stride = (int64_t)gridDim.x * (kSwThreads / 64);
    for (int64_t r = (int64_t)blockIdx.x * (kSwThreads / 64) + (threadIdx.x >> 6); r < rows; r += stride) {
        const int n = (int)(r / (ho * wo)), rem = (int)(r - (int64_t)n * ho * wo), oy = rem / wo, ox = rem - oy * wo;
        LnRow row;
#pragma unroll
        for (int i = 0; i < kRowQuads; ++i) {
            const int q = lane + 64 * i;
            row.v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (q >= nq) continue;
            const int part = q / cq, iy = 2 * oy + (part & 1), ix = 2 * ox + (part >> 1);
            if (iy < h && ix < w)
                row.v[i] = *reinterpret_cast<const float4 *>(x + (((int64_t)n * h + iy) * w + ix) * c + 4 * (q - part * cq));
        }
        ln_row_stats(nq, lane, 1.f / (float)(4 * c), eps, row);
        ln_row_write<F32OUT>(row, gamma, beta, nullptr, nq, lane, out + r * 4 * c * (F32OUT ? 4 : 2), nullptr);
    }
}

// ------------------------------------------------------------------------------------------------------ attention
struct SwAttn {
    const char *qkv;      // rows [M][3 C], compute dtype
    const float *bias;    // [3 C]
    const float *table;   // [heads][N][N]
    char *out;            // rows [M][C], compute dtype
    int batch, h, w, c, ph, pw, nwx, nwy, sh, sw;   // padded size, windows per axis, the shift left on each axis
};

template <bool F32, int WS>
struct SwCfg {
    static constexpr int kN = WS * WS;                          // 49 | 144 tokens
    static constexpr int kNQ = (kN + 15) / 16 * 16;             // 64 | 144 query rows: whole 16-row tiles
    static constexpr int kNK = (kN + 31) / 32 * 32;             // 64 | 160 keys: whole 32-key steps of the second product
    static constexpr int kRow = F32 ? (kSwHd + 4) * 4 : (kSwHd + 8) * 2;   // bytes per q / k (/ fp32 v) row in LDS: 144 | 80
    static constexpr int kVtRow = (kNK + 8) * 2;                // bytes per V^T row (16-bit): 144 | 336
    static constexpr int kQ = 0, kK = kNQ * kRow, kV = kK + kNK * kRow;
    static constexpr int kIdx = kV + (F32 ? kNK * kRow : kSwHd * kVtRow);
    static constexpr int kLds = kIdx + 2 * kNK * 4;             // + the tokens' row index and mask region
};

__device__ __forceinline__ sw_f32x4_t sw_mfma_f32(float a, float b, sw_f32x4_t c)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

template <bool F32, int WS>
__global__ void __launch_bounds__(kSwThreads) swin_attention_kernel(SwAttn a)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    using Cfg = SwCfg<F32, WS>;
    constexpr int N = Cfg::kN, NQ = Cfg::kNQ, NK = Cfg::kNK, KT = NK / 16, ESZ = F32 ? 4 : 2;
    constexpr int kPieces = F32 ? 8 : 4, kPer = F32 ? 4 : 8;    // 16-byte pieces per 32-wide head slice, values per piece
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int t16 = lane & 15, g = lane >> 4;
    const int head = blockIdx.y;
    const int per_img = a.nwx * a.nwy, n = blockIdx.x / per_img, wi = blockIdx.x - n * per_img;
    const int wy = wi / a.nwx, wx = wi - wy * a.nwx;
    int *rowi = reinterpret_cast<int *>(lds + Cfg::kIdx);       // [NK]: the token's row of qkv, -1 = a token of the padding
    int *region = rowi + NK;                                    // [NK]: 3 * row region + column region

    for (int t = tid; t < NK; t += kSwThreads) {
        int ri = -2, rg = 0;
        if (t < N) {
            const int ty = t / WS, tx = t - ty * WS;
            const int cy = wy * WS + ty, cx = wx * WS + tx;     // in the rolled frame
            int py = cy + a.sh, px = cx + a.sw;                 // in the padded map
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

    // q | k | v of this head, 16 bytes per item; a padded token carries the bias, a row past N zeros
    for (int i = tid; i < NK * 3 * kPieces; i += kSwThreads) {
        const int t = i / (3 * kPieces), rem = i - t * 3 * kPieces, part = rem / kPieces, piece = rem - part * kPieces;
        const int col = part * a.c + head * kSwHd + piece * kPer;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (t < N) {
            const int ri = rowi[t];
            if (ri >= 0) {
                v = *reinterpret_cast<const uint4 *>(a.qkv + ((int64_t)ri * 3 * a.c + col) * ESZ);
            } else if (F32) {
                v = *reinterpret_cast<const uint4 *>(a.bias + col);
            } else {
                const float4 b0 = *reinterpret_cast<const float4 *>(a.bias + col), b1 = *reinterpret_cast<const float4 *>(a.bias + col + 4);
                v = make_uint4(pack_act2(b0.x, b0.y), pack_act2(b0.z, b0.w), pack_act2(b1.x, b1.y), pack_act2(b1.z, b1.w));
            }
        }
        if (part == 0) {
            if (t < NQ) *reinterpret_cast<uint4 *>(lds + Cfg::kQ + t * Cfg::kRow + piece * 16) = v;
        } else if (part == 1 || F32) {
            *reinterpret_cast<uint4 *>(lds + (part == 1 ? Cfg::kK : Cfg::kV) + t * Cfg::kRow + piece * 16) = v;
        } else {                                                // 16-bit v goes in transposed: V^T [32][NK]
            uint16_t *vt = reinterpret_cast<uint16_t *>(lds + Cfg::kV);
            const uint32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                vt[(piece * 8 + 2 * j) * (Cfg::kVtRow / 2) + t] = (uint16_t)(e[j] & 0xffffu);
                vt[(piece * 8 + 2 * j + 1) * (Cfg::kVtRow / 2) + t] = (uint16_t)(e[j] >> 16);
            }
        }
    }
    __syncthreads();

    const bool masked = a.sh > 0 || a.sw > 0;                   // (uniform)
    const float scale = 0.17677669529663687f;                   // 32^-0.5
    for (int qt = wave; qt < NQ / 16; qt += kSwThreads / 64) {
        const int qi = 16 * qt + t16;                           // this lane's query
        sw_f32x4_t s[KT];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) s[kt] = sw_f32x4_t{0.f, 0.f, 0.f, 0.f};
        // S^T = K Q^T: s[kt][r] = score of query qi and key 16 kt + 4 g + r
        if (F32) {
            float qf[8];
#pragma unroll
            for (int st = 0; st < 8; ++st) qf[st] = *reinterpret_cast<const float *>(lds + Cfg::kQ + qi * Cfg::kRow + (4 * st + g) * 4);
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int st = 0; st < 8; ++st) {
                    const float kf = *reinterpret_cast<const float *>(lds + Cfg::kK + (16 * kt + t16) * Cfg::kRow + (4 * st + g) * 4);
                    s[kt] = sw_mfma_f32(kf, qf[st], s[kt]);
                }
        } else {
            const uint4 qf = *reinterpret_cast<const uint4 *>(lds + Cfg::kQ + qi * Cfg::kRow + g * 16);
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                const uint4 kf = *reinterpret_cast<const uint4 *>(lds + Cfg::kK + (16 * kt + t16) * Cfg::kRow + g * 16);
                s[kt] = mfma_act_16x16x32(kf, qf, s[kt]);
            }
        }
        // + bias (+ mask); a key row past N is no token: out of the softmax
        const int qc = min(qi, N - 1);                          // (a query row past N computes a row that is dropped)
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
        // O^T = V^T P^T: o[dt][r] = output channel 16 dt + 4 g + r of query qi
        sw_f32x4_t o[2] = {sw_f32x4_t{0.f, 0.f, 0.f, 0.f}, sw_f32x4_t{0.f, 0.f, 0.f, 0.f}};
        if (F32) {
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = s[kt][r] * inv;
                    const char *vrow = lds + Cfg::kV + (16 * kt + 4 * g + r) * Cfg::kRow;
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt)
                        o[dt] = sw_mfma_f32(*reinterpret_cast<const float *>(vrow + (16 * dt + t16) * 4), p, o[dt]);
                }
        } else {
#pragma unroll
            for (int u = 0; u < KT / 2; ++u) {                   // lane group g holds keys {4g .. 4g+3, 16+4g .. 16+4g+3} of a 32-key block
                const uint4 pf = make_uint4(pack_act2(s[2 * u][0] * inv, s[2 * u][1] * inv), pack_act2(s[2 * u][2] * inv, s[2 * u][3] * inv),
                                            pack_act2(s[2 * u + 1][0] * inv, s[2 * u + 1][1] * inv),
                                            pack_act2(s[2 * u + 1][2] * inv, s[2 * u + 1][3] * inv));
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const char *vrow = lds + Cfg::kV + (16 * dt + t16) * Cfg::kVtRow + (32 * u + 4 * g) * 2;
                    const uint2 lo = *reinterpret_cast<const uint2 *>(vrow), hi = *reinterpret_cast<const uint2 *>(vrow + 32);
                    o[dt] = mfma_act_16x16x32(make_uint4(lo.x, lo.y, hi.x, hi.y), pf, o[dt]);
                }
            }
        }
        const int ri = qi < N ? rowi[qi] : -1;
        if (ri < 0) continue;                                    // a padded token's (or tile row's) output is dropped
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            char *dst = a.out + ((int64_t)ri * a.c + head * kSwHd + 16 * dt + 4 * g) * ESZ;
            if (F32) *reinterpret_cast<float4 *>(dst) = make_float4(o[dt][0], o[dt][1], o[dt][2], o[dt][3]);
            else *reinterpret_cast<uint2 *>(dst) = make_uint2(pack_act2(o[dt][0], o[dt][1]), pack_act2(o[dt][2], o[dt][3]));
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ host
int check_shape(const char *what, const sdetr_swin_op &o, int precision)
{
    return check_rows_shape(what, o.batch, o.height, o.width, o.in_channels, precision);
}

// a GEMM op (kinds 0 .. 2) as the conv kernel's arguments
int make_gemm(const sdetr_swin_op &o, int precision, BConv &c)
{
    const char *what = "sdetr_swin (GEMM)";
    if (int rc = check_shape(what, o, precision)) return rc;
    if (!o.x || !o.weight || !o.bias || !o.out) return fail("%s: null tensor", what);
    if (o.out_channels < 1) return fail("%s: bad out_channels %d", what, o.out_channels);
    if (o.kernel_size < 1 || o.kernel_size > 4 || o.stride != o.kernel_size)
        return fail("%s: a patchify conv has kernel == stride in 1 .. 4 (got kernel %d, stride %d)", what, o.kernel_size, o.stride);
    if (o.x_nchw == 0 && o.in_channels % 32)
        return fail("%s: a channels-last input needs in_channels %% 32 == 0 (got %d)", what, o.in_channels);
    if (o.kind != 0 && (o.residual || o.out_nchw || o.x_nchw || o.kernel_size != 1))
        return fail("%s: only the linear epilogue takes a residual / the NCHW canvas / a patch / writes the NCHW copy", what);
    if (!all_aligned16(o.x, o.weight, o.bias, o.out, o.residual, o.out_nchw, o.aux, o.row_scale))
        return fail("%s: tensors must be 16-byte aligned", what);
    if ((o.kind != 1 && o.aux) || (o.kind != 0 && o.row_scale))
        return fail("%s: aux belongs to the GELU epilogue (kind 1), row_scale to the linear one (kind 0)", what);
    if (o.height < o.kernel_size || o.width < o.kernel_size) return fail("%s: empty output", what);
    const ConvGeom g = {o.x, o.weight, o.bias, o.residual, o.out, o.batch, o.in_channels, o.height, o.width, o.out_channels,
                        o.kernel_size, o.stride, 0, out_hw(o.height, o.kernel_size, o.stride, 0),
                        out_hw(o.width, o.kernel_size, o.stride, 0), o.x_nchw, o.splits};
    if (int rc = fill_conv(what, g, precision, c)) return rc;
    c.out_nchw = o.out_nchw;
    c.aux = reinterpret_cast<char *>(o.aux);
    c.q = o.row_scale;
    return 0;
}

int run_gemm(hipStream_t s, const sdetr_swin_op &o, int precision, void *ws, int64_t ws_bytes)
{
    BConv c;
    if (int rc = make_gemm(o, precision, c)) return rc;
    if (conv_workspace(c) > ws_bytes || (conv_workspace(c) && !ws))
        return fail("sdetr_swin (GEMM): workspace of %lld bytes is too small (%lld needed)", (long long)ws_bytes,
                    (long long)conv_workspace(c));
    c.partial = reinterpret_cast<float *>(ws);
    const bool x3 = precision == 0;
    if (o.kind == 1 && o.aux) launch_rows_gemm<6>(s, c, x3);
    else if (o.kind == 1) launch_rows_gemm<1>(s, c, x3);
    else if (o.kind == 2) launch_rows_gemm<5>(s, c, x3);
    else if (o.row_scale) launch_gemm<7>(s, c, x3, o.x_nchw != 0);
    else launch_gemm<2>(s, c, x3, o.x_nchw != 0);
    return check_launch("sdetr_swin (GEMM)");
}

int check_ln(const sdetr_swin_op &o, int precision)
{
    return check_ln_rows("sdetr_swin (LayerNorm)", o.batch, o.height, o.width, o.in_channels, precision, o.x, o.gamma, o.beta, o.out);
}

int run_ln(hipStream_t s, const sdetr_swin_op &o, int precision)
{
    if (int rc = check_ln(o, precision)) return rc;
    launch_ln_rows(s, precision == 0 || o.out_f32, o.x, o.gamma, o.beta, nullptr, (int64_t)o.batch * o.height * o.width,
                   o.in_channels, o.eps, o.out, nullptr);
    return check_launch("sdetr_swin (LayerNorm)");
}

int check_merge(const sdetr_swin_op &o, int precision)
{
    const char *what = "sdetr_swin (patch merging)";
    if (int rc = check_shape(what, o, precision)) return rc;
    if ((4 * o.in_channels) % 32 || 4 * o.in_channels > kRowMaxC)
        return fail("%s: 4 C must be a multiple of 32 up to %d (got C = %d)", what, kRowMaxC, o.in_channels);
    if (!o.x || !o.gamma || !o.beta || !o.out) return fail("%s: null tensor", what);
    if (!all_aligned16(o.x, o.gamma, o.beta, o.out))
        return fail("%s: tensors must be 16-byte aligned", what);
    return 0;
}

int run_merge(hipStream_t s, const sdetr_swin_op &o, int precision)
{
    if (int rc = check_merge(o, precision)) return rc;
    const int64_t rows = (int64_t)o.batch * ((o.height + 1) / 2) * ((o.width + 1) / 2);
    const unsigned blocks = (unsigned)std::min<int64_t>((rows + 3) / 4, 16384);
    const float *x = reinterpret_cast<const float *>(o.x);
    if (precision == 0)
        hipLaunchKernelGGL(swin_merge_ln_kernel<true>, dim3(blocks), dim3(kSwThreads), 0, s, x, o.gamma, o.beta, o.batch, o.height,
                           o.width, o.in_channels, o.eps, reinterpret_cast<char *>(o.out));
    else
        hipLaunchKernelGGL(swin_merge_ln_kernel<false>, dim3(blocks), dim3(kSwThreads), 0, s, x, o.gamma, o.beta, o.batch, o.height,
                           o.width, o.in_channels, o.eps, reinterpret_cast<char *>(o.out));
    return check_launch("sdetr_swin (patch merging)");
}

int make_attention(const sdetr_swin_op &o, int precision, SwAttn &a)
{
    const char *what = "sdetr_swin (window attention)";
    if (int rc = check_shape(what, o, precision)) return rc;
    if (o.in_channels % 32) return fail("%s: channels must be a multiple of 32 (got %d)", what, o.in_channels);
    if (o.heads < 1 || o.heads > 65535 || (int64_t)o.heads * kSwHd != o.in_channels)
        return fail("%s: the head dimension must be %d (got %d channels over %d heads)", what, kSwHd, o.in_channels, o.heads);
    if (o.window != 7 && o.window != 12) return fail("%s: window must be 7 or 12 (got %d)", what, o.window);
    if (o.shift < 0 || o.shift >= o.window) return fail("%s: shift must lie in [0, window) (got %d)", what, o.shift);
    if (!o.x || !o.bias || !o.table || !o.out) return fail("%s: null tensor", what);
    if (o.x == o.out) return fail("%s: x must not alias out", what);
    if (!all_aligned16(o.x, o.bias, o.table, o.out))
        return fail("%s: tensors must be 16-byte aligned", what);
    a.qkv = reinterpret_cast<const char *>(o.x);
    a.bias = o.bias;
    a.table = o.table;
    a.out = reinterpret_cast<char *>(o.out);
    a.batch = o.batch;
    a.h = o.height;
    a.w = o.width;
    a.c = o.in_channels;
    a.nwy = (o.height + o.window - 1) / o.window;
    a.nwx = (o.width + o.window - 1) / o.window;
    a.ph = a.nwy * o.window;
    a.pw = a.nwx * o.window;
    a.sh = o.window >= a.ph ? 0 : o.shift;      // per axis: no shift where one window spans the padded map
    a.sw = o.window >= a.pw ? 0 : o.shift;
    if ((int64_t)o.batch * a.nwx * a.nwy >= (int64_t(1) << 31)) return fail("%s: too many windows", what);
    return 0;
}

template <bool F32, int WS>
void launch_attention(hipStream_t s, const SwAttn &a, int heads)
{
    static DeviceOnce once;
    constexpr int bytes = SwCfg<F32, WS>::kLds;   // 15 360 | 28 160 (window 7), 36 352 | 68 096 (window 12): 16-bit | fp32
    static_assert(bytes <= 80 * 1024, "two workgroups of the window attention fit a CU's LDS");
    allow_dynamic_lds(swin_attention_kernel<F32, WS>, once, bytes);
    hipLaunchKernelGGL((swin_attention_kernel<F32, WS>), dim3((unsigned)(a.batch * a.nwx * a.nwy), (unsigned)heads),
                       dim3(kSwThreads), bytes, s, a);
}

int run_attention(hipStream_t s, const sdetr_swin_op &o, int precision)
{
    SwAttn a;
    if (int rc = make_attention(o, precision, a)) return rc;
    if (precision == 0 && o.window == 7) launch_attention<true, 7>(s, a, o.heads);
    else if (precision == 0) launch_attention<true, 12>(s, a, o.heads);
    else if (o.window == 7) launch_attention<false, 7>(s, a, o.heads);
    else launch_attention<false, 12>(s, a, o.heads);
    return check_launch("sdetr_swin (window attention)");
}

// validation of one op without a launch; `need` receives its workspace bytes
int check_op(const sdetr_swin_op &o, int precision, int64_t &need)
{
    need = 0;
    if (o.kind >= 0 && o.kind <= 2) {
        BConv c;
        if (int rc = make_gemm(o, precision, c)) return rc;
        need = conv_workspace(c);
        return 0;
    }
    if (o.kind >= 3 && o.kind <= 5 && (o.aux || o.row_scale))
        return fail("sdetr_swin: aux / row_scale belong to the GEMM kinds (got kind %d)", o.kind);
    if (o.kind == 3) return check_ln(o, precision);
    if (o.kind == 4) {
        SwAttn a;
        return make_attention(o, precision, a);
    }
    if (o.kind == 5) return check_merge(o, precision);
    return fail("sdetr_swin: unknown op kind %d", o.kind);
}

int run_op(hipStream_t s, const sdetr_swin_op &o, int precision, void *ws, int64_t ws_bytes)
{
    if (o.kind >= 0 && o.kind <= 2) return run_gemm(s, o, precision, ws, ws_bytes);
    if (o.kind == 3) return run_ln(s, o, precision);
    if (o.kind == 4) return run_attention(s, o, precision);
    if (o.kind == 5) return run_merge(s, o, precision);
    return fail("sdetr_swin: unknown op kind %d", o.kind);
}

}  // namespace
}  // namespace sdetr

using namespace sdetr;

using SwinPlan = Plan<sdetr_swin_op, check_op, run_op>;

extern "C" int64_t sdetr_swin_workspace_bytes(const sdetr_swin_op *ops, int n_ops, int precision)
{
    return SwinPlan::workspace_bytes(ops, n_ops, precision);
}

extern "C" int sdetr_swin_op_run(sdetr_stream_t stream, const sdetr_swin_op *op, int precision, void *workspace,
                                 int64_t workspace_bytes)
{
    return SwinPlan::op_run("sdetr_swin", stream, op, precision, workspace, workspace_bytes);
}

extern "C" int sdetr_swin_run(sdetr_stream_t stream, const sdetr_swin_op *ops, int n_ops, int precision, void *workspace,
                              int64_t workspace_bytes)
{
    return SwinPlan::run("sdetr_swin", stream, ops, n_ops, precision, workspace, workspace_bytes);
}

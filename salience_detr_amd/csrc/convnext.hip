// The ConvNeXt backbone (reference models/backbones/convnext.py), eval mode.  The residual stream is channels-last fp32
// [B, H, W, C] in every precision (under autocast the reference's stream stays fp32 too: layer_scale is fp32 and
// `result += input`); the "compute dtype" (fp32, or the library's 16-bit type) is the type of the GEMM A operands.
//
//   convnext_dwconv_ln_kernel   depthwise 7x7 (padding 3) + bias + LayerNorm over C in ONE launch: a workgroup owns a tile
//                               of 8 x TH pixels and all of its channels; it walks the channels in chunks of CC, each
//                               chunk's input rows + halo and its 49 taps staged in LDS, lanes along C (4 channels each),
//                               a lane's strip of SW pixels sliding over the staged row; the pre-norm values of the whole
//                               tile stay in LDS (fp32), the statistics are two-pass sums over them (one wave per pixel),
//                               the normalised rows leave in the compute dtype.  TH, CC and SW follow C (tile_for).
//   ln_rows_kernel              LayerNorm over C of fp32 rows (the stem's LayerNorm2d and the one in front of each
//                               down-sampler): backbone_rows_core.h's, fp32 or compute-dtype output
//   the GEMMs                   backbone_conv_core.h's implicit-GEMM kernel with kernel == stride, padding 0: a Linear is
//                               its 1x1 case over rows, the down-sampler its 2x2 stride-2 case, the stem its 4x4 stride-4
//                               case on the fp32 NCHW canvas; epilogue gelu(acc + b) (EPI 1) or acc + b (+ fp32 residual)
//                               with the fp32 NCHW copy of a returned stage (EPI 2).  Weights: sdetr_backbone_pack.
// A training forward (convnext_backward.hip is its backward) sets `aux` / `row_scale`: the depthwise launch also writes its
// pre-norm fp32 values, Linear 1 its pre-GELU values (EPI 6), Linear 2 scales acc + b per sample (EPI 7).  Null: as above.
// The row LayerNorm, the host checks of a rows op and the plan entry points are backbone_rows_core.h's.
// No atomics; a split reduction is summed in split order through the workspace.
#include "backbone_rows_core.h"

namespace sdetr {
namespace {

constexpr int kCnThreads = 256;
constexpr int kCnTW = 8;                      // tile width in pixels
constexpr int kCnPreBytes = 96 * 1024;        // the tile's pre-norm values
constexpr int kCnLdsBytes = 150000;           // pre-norm + one chunk's rows, halo and taps
constexpr int kCnMaxC = 3072;                 // a 1 x 8 tile at the pre-norm budget

struct CnTile {
    int th, cc, sw, lds;
};
// Per C: the tallest tile whose pre-norm values fit, the widest chunk that fits beside them, and the strip width that
// still gives every thread an item (items = TH * (8 / SW) * CC / 4).
//   C      8 x TH  pre-norm B   CC    chunk B (rows + halo + taps)   SW
//   96     8x16    49 152       64    91 392                         8
//   192    8x16    98 304       32    45 696                         4
//   384    8x8     98 304       32    31 360                         2
//   768    8x4     98 304       64    48 384                         2
//   1536   8x2     98 304       64    41 216                         1
bool tile_for(int c, CnTile &t)
{
    if (c < 32 || c % 32 || c > kCnMaxC) return false;
    t.th = 16;
    while (t.th > 1 && kCnTW * t.th * c * 4 > kCnPreBytes) t.th >>= 1;
    const int pre = kCnTW * t.th * c * 4, per_channel = (t.th + 6) * (kCnTW + 6) * 4 + 49 * 4;
    t.cc = 128;
    while (t.cc > 32 && (t.cc > c || pre + t.cc * per_channel > kCnLdsBytes)) t.cc >>= 1;
    t.sw = 8;
    while (t.sw > 1 && t.th * (kCnTW / t.sw) * (t.cc / 4) < kCnThreads) t.sw >>= 1;
    t.lds = pre + t.cc * per_channel;
    return t.lds <= kCnLdsBytes;
}

struct CnDw {
    const float *x;       // [B, H, W, C] fp32
    const float *taps;    // [49][C]
    const float *bias, *gamma, *beta;
    char *out;            // [B, H, W, C] compute dtype
    float *pre_out;       // [B, H, W, C] fp32: the values before the LayerNorm (a training forward), or null
    int batch, h, w, c, th, cc, tiles_x, tiles_y;
    float eps;
};

template <int SW, bool F32OUT>
__global__ void __launch_bounds__(kCnThreads) convnext_dwconv_ln_kernel(CnDw a)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tiles = a.tiles_x * a.tiles_y;
    const int n = blockIdx.x / tiles, trem = blockIdx.x - n * tiles, ty = trem / a.tiles_x, tx = trem - ty * a.tiles_x;
    const int y0 = ty * a.th, x0 = tx * kCnTW;
    const int P = kCnTW * a.th, HR = a.th + 6, HC = kCnTW + 6;
    float *pre = reinterpret_cast<float *>(lds);            // [P][C]
    float *halo = pre + P * a.c;                            // [HR][HC][cc]
    float *tap = halo + HR * HC * a.cc;                     // [49][cc]
    const float *img = a.x + (int64_t)n * a.h * a.w * a.c;

    for (int c0 = 0; c0 < a.c; c0 += a.cc) {
        const int cc = min(a.cc, a.c - c0), q4 = cc >> 2;   // (C % 32 == 0: whole quads)
        __syncthreads();                                    // the previous chunk's readers are done
        for (int i = tid; i < HR * HC * q4; i += kCnThreads) {
            const int q = i % q4, pix = i / q4, hx = pix % HC, hy = pix / HC;
            const int iy = y0 + hy - 3, ix = x0 + hx - 3;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((unsigned)iy < (unsigned)a.h && (unsigned)ix < (unsigned)a.w)
                v = *reinterpret_cast<const float4 *>(img + ((int64_t)iy * a.w + ix) * a.c + c0 + 4 * q);
            *reinterpret_cast<float4 *>(halo + pix * a.cc + 4 * q) = v;
        }
        for (int i = tid; i < 49 * q4; i += kCnThreads) {
            const int q = i % q4, t = i / q4;
            *reinterpret_cast<float4 *>(tap + t * a.cc + 4 * q) =
                *reinterpret_cast<const float4 *>(a.taps + (int64_t)t * a.c + c0 + 4 * q);
        }
        __syncthreads();
        constexpr int kStrips = kCnTW / SW;
        for (int item = tid; item < a.th * kStrips * q4; item += kCnThreads) {
            const int q = item % q4, rest = item / q4, s = rest % kStrips, y = rest / kStrips;
            const float4 b = *reinterpret_cast<const float4 *>(a.bias + c0 + 4 * q);
            float4 acc[SW];
#pragma unroll
            for (int i = 0; i < SW; ++i) acc[i] = b;
            for (int ky = 0; ky < 7; ++ky) {
                const float *row = halo + ((y + ky) * HC + s * SW) * a.cc + 4 * q;
                float4 in[SW + 6], wt[7];
#pragma unroll
                for (int i = 0; i < SW + 6; ++i) in[i] = *reinterpret_cast<const float4 *>(row + i * a.cc);
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) wt[kx] = *reinterpret_cast<const float4 *>(tap + (ky * 7 + kx) * a.cc + 4 * q);
#pragma unroll
                for (int kx = 0; kx < 7; ++kx)
#pragma unroll
                    for (int i = 0; i < SW; ++i) {
                        acc[i].x = fmaf(in[i + kx].x, wt[kx].x, acc[i].x);
                        acc[i].y = fmaf(in[i + kx].y, wt[kx].y, acc[i].y);
                        acc[i].z = fmaf(in[i + kx].z, wt[kx].z, acc[i].z);
                        acc[i].w = fmaf(in[i + kx].w, wt[kx].w, acc[i].w);
                    }
            }
#pragma unroll
            for (int i = 0; i < SW; ++i)
                *reinterpret_cast<float4 *>(pre + (y * kCnTW + s * SW + i) * a.c + c0 + 4 * q) = acc[i];
        }
    }
    __syncthreads();

    // LayerNorm: one wave per pixel, lanes along C; mean, then the variance about it
    const int nq = a.c >> 2;
    const float inv_c = 1.f / (float)a.c;
    for (int p = wave; p < P; p += kCnThreads / 64) {
        const int py = y0 + p / kCnTW, px = x0 + p % kCnTW;
        if (py >= a.h || px >= a.w) continue;               // (uniform over the wave)
        const float *r = pre + p * a.c;
        float s = 0.f;
        for (int q = lane; q < nq; q += 64) {
            const float4 v = *reinterpret_cast<const float4 *>(r + 4 * q);
            s += (v.x + v.y) + (v.z + v.w);
        }
        const float mean = wave_sum(s) * inv_c;
        float ss = 0.f;
        for (int q = lane; q < nq; q += 64) {
            const float4 v = *reinterpret_cast<const float4 *>(r + 4 * q);
            const float dx = v.x - mean, dy = v.y - mean, dz = v.z - mean, dw = v.w - mean;
            ss += (dx * dx + dy * dy) + (dz * dz + dw * dw);
        }
        const float rstd = 1.f / sqrtf(wave_sum(ss) * inv_c + a.eps);
        const int64_t o = (((int64_t)n * a.h + py) * a.w + px) * a.c;
        for (int q = lane; q < nq; q += 64) {
            const float4 v = *reinterpret_cast<const float4 *>(r + 4 * q);
            if (a.pre_out) *reinterpret_cast<float4 *>(a.pre_out + o + 4 * q) = v;
            const float4 g = *reinterpret_cast<const float4 *>(a.gamma + 4 * q);
            const float4 be = *reinterpret_cast<const float4 *>(a.beta + 4 * q);
            const float o0 = fmaf((v.x - mean) * rstd, g.x, be.x), o1 = fmaf((v.y - mean) * rstd, g.y, be.y);
            const float o2 = fmaf((v.z - mean) * rstd, g.z, be.z), o3 = fmaf((v.w - mean) * rstd, g.w, be.w);
            if (F32OUT) *reinterpret_cast<float4 *>(a.out + (o + 4 * q) * 4) = make_float4(o0, o1, o2, o3);
            else *reinterpret_cast<uint2 *>(a.out + (o + 4 * q) * 2) = make_uint2(pack_act2(o0, o1), pack_act2(o2, o3));
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ host
int make_dw(const sdetr_convnext_op &o, int precision, CnDw &a, CnTile &t)
{
    const char *what = "sdetr_convnext (depthwise + LayerNorm)";
    if (int rc = check_rows_shape(what, o.batch, o.height, o.width, o.in_channels, precision)) return rc;
    if (!o.x || !o.weight || !o.bias || !o.gamma || !o.beta || !o.out) return fail("%s: null tensor", what);
    if (!tile_for(o.in_channels, t))
        return fail("%s: channels must be a multiple of 32 in [32, %d] (got %d)", what, kCnMaxC, o.in_channels);
    if (!all_aligned16(o.x, o.weight, o.bias, o.gamma, o.beta, o.out, o.aux))
        return fail("%s: tensors must be 16-byte aligned", what);
    if (o.row_scale) return fail("%s: row_scale belongs to kind 0", what);
    a.pre_out = reinterpret_cast<float *>(o.aux);
    a.x = reinterpret_cast<const float *>(o.x);
    a.taps = reinterpret_cast<const float *>(o.weight);
    a.bias = o.bias;
    a.gamma = o.gamma;
    a.beta = o.beta;
    a.out = reinterpret_cast<char *>(o.out);
    a.batch = o.batch;
    a.h = o.height;
    a.w = o.width;
    a.c = o.in_channels;
    a.th = t.th;
    a.cc = t.cc;
    a.tiles_x = (o.width + kCnTW - 1) / kCnTW;
    a.tiles_y = (o.height + t.th - 1) / t.th;
    a.eps = o.eps;
    if ((int64_t)a.batch * a.tiles_x * a.tiles_y >= (int64_t(1) << 31)) return fail("%s: too many tiles", what);
    return 0;
}

template <int SW, bool F32OUT>
void launch_dw_sw(hipStream_t s, const CnDw &a, const CnTile &t)
{
    static DeviceOnce once;
    allow_dynamic_lds(convnext_dwconv_ln_kernel<SW, F32OUT>, once, kCnLdsBytes);
    hipLaunchKernelGGL((convnext_dwconv_ln_kernel<SW, F32OUT>), dim3((unsigned)(a.batch * a.tiles_x * a.tiles_y)),
                       dim3(kCnThreads), t.lds, s, a);
}
template <bool F32OUT>
void launch_dw(hipStream_t s, const CnDw &a, const CnTile &t)
{
    if (t.sw == 8) launch_dw_sw<8, F32OUT>(s, a, t);
    else if (t.sw == 4) launch_dw_sw<4, F32OUT>(s, a, t);
    else if (t.sw == 2) launch_dw_sw<2, F32OUT>(s, a, t);
    else launch_dw_sw<1, F32OUT>(s, a, t);
}

int run_dw(hipStream_t s, const sdetr_convnext_op &o, int precision)
{
    CnDw a;
    CnTile t;
    if (int rc = make_dw(o, precision, a, t)) return rc;
    if (precision == 0) launch_dw<true>(s, a, t);
    else launch_dw<false>(s, a, t);
    return check_launch("sdetr_convnext (depthwise + LayerNorm)");
}

int check_ln(const sdetr_convnext_op &o, int precision)
{
    if (o.aux || o.row_scale) return fail("sdetr_convnext (LayerNorm): aux / row_scale belong to kinds 0 .. 2");
    return check_ln_rows("sdetr_convnext (LayerNorm)", o.batch, o.height, o.width, o.in_channels, precision, o.x, o.gamma, o.beta,
                         o.out);
}

int run_ln(hipStream_t s, const sdetr_convnext_op &o, int precision)
{
    if (int rc = check_ln(o, precision)) return rc;
    launch_ln_rows(s, precision == 0 || o.out_f32, o.x, o.gamma, o.beta, nullptr, (int64_t)o.batch * o.height * o.width,
                   o.in_channels, o.eps, o.out, nullptr);
    return check_launch("sdetr_convnext (LayerNorm)");
}

// a GEMM op (kind 0 / 1) as the conv kernel's arguments: kernel == stride, padding 0
int make_gemm(const sdetr_convnext_op &o, int precision, BConv &c)
{
    const char *what = "sdetr_convnext (patchify GEMM)";
    if (int rc = check_rows_shape(what, o.batch, o.height, o.width, o.in_channels, precision)) return rc;
    if (!o.x || !o.weight || !o.bias || !o.out) return fail("%s: null tensor", what);
    if (o.out_channels < 1) return fail("%s: bad out_channels %d", what, o.out_channels);
    if (o.kernel_size < 1 || o.kernel_size > 4 || o.stride != o.kernel_size)
        return fail("%s: a patchify conv has kernel == stride in 1 .. 4 (got kernel %d, stride %d)", what, o.kernel_size,
                    o.stride);
    if (o.x_nchw == 0 && o.in_channels % 32)
        return fail("%s: a channels-last input needs in_channels %% 32 == 0 (got %d)", what, o.in_channels);
    if (o.kind == 1 && (o.residual || o.out_nchw)) return fail("%s: the GELU epilogue takes no residual / NCHW copy", what);
    if (!all_aligned16(o.x, o.weight, o.aux, o.row_scale)) return fail("%s: x, weight, aux and row_scale must be 16-byte aligned", what);
    if ((o.kind == 0 && o.aux) || (o.kind == 1 && o.row_scale))
        return fail("%s: aux belongs to the GELU epilogue (kind 1), row_scale to the linear one (kind 0)", what);
    const int ho = out_hw(o.height, o.kernel_size, o.stride, 0), wo = out_hw(o.width, o.kernel_size, o.stride, 0);
    if (ho < 1 || wo < 1) return fail("%s: empty output", what);
    const ConvGeom g = {o.x, o.weight, o.bias, o.residual, o.out, o.batch, o.in_channels, o.height, o.width, o.out_channels,
                        o.kernel_size, o.stride, 0, ho, wo, o.x_nchw, o.splits};
    if (int rc = fill_conv(what, g, precision, c)) return rc;
    c.out_nchw = o.out_nchw;
    c.aux = reinterpret_cast<char *>(o.aux);
    c.q = o.row_scale;
    return 0;
}

int run_gemm(hipStream_t s, const sdetr_convnext_op &o, int precision, void *ws, int64_t ws_bytes)
{
    BConv c;
    if (int rc = make_gemm(o, precision, c)) return rc;
    if (conv_workspace(c) > ws_bytes || (conv_workspace(c) && !ws))
        return fail("sdetr_convnext (patchify GEMM): workspace of %lld bytes is too small (%lld needed)",
                    (long long)ws_bytes, (long long)conv_workspace(c));
    c.partial = reinterpret_cast<float *>(ws);
    if (o.kind == 1 && o.aux) launch_gemm<6>(s, c, precision == 0, o.x_nchw != 0);
    else if (o.kind == 1) launch_gemm<1>(s, c, precision == 0, o.x_nchw != 0);
    else if (o.row_scale) launch_gemm<7>(s, c, precision == 0, o.x_nchw != 0);
    else launch_gemm<2>(s, c, precision == 0, o.x_nchw != 0);
    return check_launch("sdetr_convnext (patchify GEMM)");
}

// validation of one op without a launch; `need` receives its workspace bytes
int check_op(const sdetr_convnext_op &o, int precision, int64_t &need)
{
    need = 0;
    if (o.kind == 0 || o.kind == 1) {
        BConv c;
        if (int rc = make_gemm(o, precision, c)) return rc;
        need = conv_workspace(c);
        return 0;
    }
    if (o.kind == 2) {
        CnDw a;
        CnTile t;
        return make_dw(o, precision, a, t);
    }
    if (o.kind == 3) return check_ln(o, precision);
    return fail("sdetr_convnext: unknown op kind %d", o.kind);
}

int run_op(hipStream_t s, const sdetr_convnext_op &o, int precision, void *ws, int64_t ws_bytes)
{
    if (o.kind == 0 || o.kind == 1) return run_gemm(s, o, precision, ws, ws_bytes);
    if (o.kind == 2) return run_dw(s, o, precision);
    if (o.kind == 3) return run_ln(s, o, precision);
    return fail("sdetr_convnext: unknown op kind %d", o.kind);
}

}  // namespace
}  // namespace sdetr

using namespace sdetr;

extern "C" int sdetr_convnext_dw_tile(int channels, int *tile_height, int *chunk_channels, int *strip_width)
{
    CnTile t;
    if (!tile_for(channels, t)) return fail("sdetr_convnext_dw_tile: channels must be a multiple of 32 in [32, %d] (got %d)",
                                            kCnMaxC, channels);
    if (tile_height) *tile_height = t.th;
    if (chunk_channels) *chunk_channels = t.cc;
    if (strip_width) *strip_width = t.sw;
    return t.lds;
}

using ConvnextPlan = Plan<sdetr_convnext_op, check_op, run_op>;

extern "C" int64_t sdetr_convnext_workspace_bytes(const sdetr_convnext_op *ops, int n_ops, int precision)
{
    return ConvnextPlan::workspace_bytes(ops, n_ops, precision);
}

extern "C" int sdetr_convnext_op_run(sdetr_stream_t stream, const sdetr_convnext_op *op, int precision, void *workspace,
                                     int64_t workspace_bytes)
{
    return ConvnextPlan::op_run("sdetr_convnext", stream, op, precision, workspace, workspace_bytes);
}

extern "C" int sdetr_convnext_run(sdetr_stream_t stream, const sdetr_convnext_op *ops, int n_ops, int precision,
                                  void *workspace, int64_t workspace_bytes)
{
    return ConvnextPlan::run("sdetr_convnext", stream, ops, n_ops, precision, workspace, workspace_bytes);
}

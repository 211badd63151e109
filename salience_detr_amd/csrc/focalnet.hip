// The FocalNet backbone (reference models/backbones/focalnet.py), eval mode.  As in convnext.hip the residual stream is
// channels-last fp32 [B, H, W, C] in every precision and the "compute dtype" (fp32, or the library's 16-bit type) is the
// type of the GEMM A operands written between launches.  Depthwise work, gates, means, LayerNorm statistics and q are fp32.
//
//   the GEMMs                 backbone_conv_core.h's implicit-GEMM kernel: f / proj / fc2 (EPI 2), fc1 + GELU (EPI 1), h with
//                             the modulation product (acc + b) * q (EPI 3, or 4 into fp32 rows), and the patch embeddings
//                             with their own stride, padding and OUTPUT size (the reference pads the input with zeros up
//                             to a multiple of the patch; out-of-range taps read zeros here, so only the size changes)
//   focal_level_kernel        ctx_l = gelu(depthwise k x k (ctx_{l-1})), ctx_all (+)= ctx_l * gate_l; a workgroup owns
//                             8 x 16 pixels x 32 channels, its input rows + halo and its k * k taps staged in LDS, lanes
//                             along C (4 channels each), a lane's strip of 4 pixels sliding over the staged row; the last
//                             level also leaves the tile's per-channel sums of ctx_L in the workspace
//   focal_mean_kernel         the tile sums added in tile order: gelu(mean over H x W) per image and channel
//   focal_finish_kernel       ctx_all + gelu(mean) * gate_L -> the A operand of h, compute dtype
//   ln_rows_kernel            LayerNorm over C of fp32 rows (+ fp32 residual): fp32 or compute-dtype rows, and a 16-bit copy
//                             (backbone_rows_core.h's)
//   focal_ln_nchw_kernel      LayerNorm over C of the stage's stream -> fp32 NCHW, 64 pixels x 64 channels through LDS (the
//                             shared row statistics, its own transpose)
//   focal_cast_kernel         fp32 rows -> 16-bit rows (the pre-LN stream in front of a down-sampler, 16-bit mode)
// The row LayerNorm, the host checks of a rows op and the plan entry points are backbone_rows_core.h's.
// No atomics; every reduction across workgroups goes through the workspace in a fixed order.
#include "backbone_rows_core.h"

namespace sdetr {
namespace {

constexpr int kFnThreads = 256;
constexpr int kFnTW = 8, kFnTH = 16;          // pixel tile of the focal level
constexpr int kFnCC = 32;                     // its channel chunk
constexpr int kFnSW = 4;                      // strip width: 16 rows x 2 strips x 8 quads = 256 items

struct FnLevel {
    const float *x;       // ctx_{l-1}: pixel m, channel c at x[m * x_ld + c]
    const float *taps;    // [k * k][C]
    const float *gate;    // gate_l of pixel m at gate[m * gate_ld]
    float *ctx;           // ctx_l [M][C], or null
    float *all;           // ctx_all [M][C]
    float *sums;          // [B][tiles][C], or null
    int64_t x_ld, gate_ld;
    int batch, h, w, c, tiles_x, tiles_y, accumulate;
};

template <int K>
__global__ void __launch_bounds__(kFnThreads) focal_level_kernel(FnLevel a)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    constexpr int R = K / 2, HR = kFnTH + K - 1, HC = kFnTW + K - 1, Q4 = kFnCC / 4;
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x, n = blockIdx.z;
    const int y0 = ty * kFnTH, x0 = tx * kFnTW, c0 = blockIdx.y * kFnCC;
    float *halo = reinterpret_cast<float *>(lds);          // [HR][HC][32]
    float *tap = halo + HR * HC * kFnCC;                   // [K * K][32]
    const int64_t img = (int64_t)n * a.h * a.w;

    for (int i = tid; i < HR * HC * Q4; i += kFnThreads) {
        const int q = i % Q4, pix = i / Q4, hx = pix % HC, hy = pix / HC;
        const int iy = y0 + hy - R, ix = x0 + hx - R;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((unsigned)iy < (unsigned)a.h && (unsigned)ix < (unsigned)a.w)
            v = *reinterpret_cast<const float4 *>(a.x + (img + (int64_t)iy * a.w + ix) * a.x_ld + c0 + 4 * q);
        *reinterpret_cast<float4 *>(halo + pix * kFnCC + 4 * q) = v;
    }
    for (int i = tid; i < K * K * Q4; i += kFnThreads) {
        const int q = i % Q4, t = i / Q4;
        *reinterpret_cast<float4 *>(tap + t * kFnCC + 4 * q) =
            *reinterpret_cast<const float4 *>(a.taps + (int64_t)t * a.c + c0 + 4 * q);
    }
    __syncthreads();

    const int q = tid % Q4, rest = tid / Q4, s = rest % (kFnTW / kFnSW), y = rest / (kFnTW / kFnSW);
    float4 acc[kFnSW];
#pragma unroll
    for (int i = 0; i < kFnSW; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int ky = 0; ky < K; ++ky) {
        const float *row = halo + ((y + ky) * HC + s * kFnSW) * kFnCC + 4 * q;
        float4 in[kFnSW + K - 1], wt[K];
#pragma unroll
        for (int i = 0; i < kFnSW + K - 1; ++i) in[i] = *reinterpret_cast<const float4 *>(row + i * kFnCC);
#pragma unroll
        for (int kx = 0; kx < K; ++kx) wt[kx] = *reinterpret_cast<const float4 *>(tap + (ky * K + kx) * kFnCC + 4 * q);
#pragma unroll
        for (int kx = 0; kx < K; ++kx)
#pragma unroll
            for (int i = 0; i < kFnSW; ++i) {
                acc[i].x = fmaf(in[i + kx].x, wt[kx].x, acc[i].x);
                acc[i].y = fmaf(in[i + kx].y, wt[kx].y, acc[i].y);
                acc[i].z = fmaf(in[i + kx].z, wt[kx].z, acc[i].z);
                acc[i].w = fmaf(in[i + kx].w, wt[kx].w, acc[i].w);
            }
    }

    float4 part = make_float4(0.f, 0.f, 0.f, 0.f);         // the strip's valid pixels, left to right
    const int py = y0 + y;
#pragma unroll
    for (int i = 0; i < kFnSW; ++i) {
        const int px = x0 + s * kFnSW + i;
        if (py >= a.h || px >= a.w) continue;
        const int64_t m = img + (int64_t)py * a.w + px, e = m * a.c + c0 + 4 * q;
        const float4 g = make_float4(gelu_erf(acc[i].x), gelu_erf(acc[i].y), gelu_erf(acc[i].z), gelu_erf(acc[i].w));
        if (a.ctx) *reinterpret_cast<float4 *>(a.ctx + e) = g;
        const float gt = a.gate[m * a.gate_ld];
        float4 o = make_float4(g.x * gt, g.y * gt, g.z * gt, g.w * gt);
        if (a.accumulate) {
            const float4 old = *reinterpret_cast<const float4 *>(a.all + e);
            o = make_float4(old.x + o.x, old.y + o.y, old.z + o.z, old.w + o.w);
        }
        *reinterpret_cast<float4 *>(a.all + e) = o;
        part = make_float4(part.x + g.x, part.y + g.y, part.z + g.z, part.w + g.w);
    }
    if (a.sums) {                                          // (uniform) the strips' sums added in strip order
        __syncthreads();                                   // the halo's readers are done: its space holds the partials
        float *red = halo;                                 // [32 strips][32]
        *reinterpret_cast<float4 *>(red + rest * kFnCC + 4 * q) = part;
        __syncthreads();
        if (tid < kFnCC) {
            float t = 0.f;
            for (int r = 0; r < kFnThreads / Q4; ++r) t += red[r * kFnCC + tid];
            a.sums[((int64_t)n * gridDim.x + blockIdx.x) * a.c + c0 + tid] = t;
        }
    }
}

// gelu(mean over H x W) per (image, channel): the tile sums in tile order
__global__ void __launch_bounds__(kFnThreads) focal_mean_kernel(const float *sums, int tiles, int c, float inv_hw, float *mean)
{
    const int ch = blockIdx.x * kFnThreads + threadIdx.x, n = blockIdx.y;
    if (ch >= c) return;
    const float *p = sums + (int64_t)n * tiles * c + ch;
    float t = 0.f;
    for (int i = 0; i < tiles; ++i) t += p[(int64_t)i * c];
    mean[(int64_t)n * c + ch] = gelu_erf(t * inv_hw);
}

// ctx_all + gelu(mean) * gate_L -> the A operand of h; one quad of channels per thread
template <bool F32OUT>
__global__ void __launch_bounds__(kFnThreads) focal_finish_kernel(const float *all, const float *mean, const float *gate,
                                                                  int64_t gate_ld, int64_t rows, int hw, int c, char *out)
{
    const int nq = c >> 2;
    const int64_t total = rows * nq, stride = (int64_t)gridDim.x * kFnThreads;
    for (int64_t i = (int64_t)blockIdx.x * kFnThreads + threadIdx.x; i < total; i += stride) {
        const int64_t m = i / nq;
        const int q = (int)(i - m * nq), n = (int)(m / hw);
        const float4 v = *reinterpret_cast<const float4 *>(all + m * c + 4 * q);
        const float4 g = *reinterpret_cast<const float4 *>(mean + (int64_t)n * c + 4 * q);
        const float gt = gate[m * gate_ld];
        const float o0 = fmaf(g.x, gt, v.x), o1 = fmaf(g.y, gt, v.y), o2 = fmaf(g.z, gt, v.z), o3 = fmaf(g.w, gt, v.w);
        if (F32OUT) *reinterpret_cast<float4 *>(out + (m * c + 4 * q) * 4) = make_float4(o0, o1, o2, o3);
        else *reinterpret_cast<uint2 *>(out + (m * c + 4 * q) * 2) = make_uint2(pack_act2(o0, o1), pack_act2(o2, o3));
    }
}

// LayerNorm over C of x [B][HW][C] -> fp32 NCHW [B][C][HW]: a workgroup owns 64 pixels of one image; one wave per row for
// the statistics, then 64 channels at a time normalised into an LDS tile and written along the pixels
__global__ void __launch_bounds__(kFnThreads) focal_ln_nchw_kernel(const float *x, const float *gamma, const float *beta,
                                                                   int hw, int c, float eps, float *out)
{
    __shared__ float tile[64][65];
    __shared__ float stat[64][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = blockIdx.y, p0 = blockIdx.x * 64;
    const int np = min(64, hw - p0), nq = c >> 2;
    const float *img = x + ((int64_t)n * hw + p0) * c;
    for (int p = wave; p < np; p += kFnThreads / 64) {
        LnRow row;
        ln_row_load(img + (int64_t)p * c, nq, lane, row);
        ln_row_stats(nq, lane, 1.f / (float)c, eps, row);
        if (lane == 0) stat[p][0] = row.mean, stat[p][1] = row.rstd;
    }
    __syncthreads();
    for (int c0 = 0; c0 < c; c0 += 64) {
        const int q = tid & 15, nc = min(64, c - c0);      // (C % 32 == 0: whole quads)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = (tid >> 4) + 16 * j;
            if (p >= np || 4 * q >= nc) continue;
            const float4 v = *reinterpret_cast<const float4 *>(img + (int64_t)p * c + c0 + 4 * q);
            const float4 g = *reinterpret_cast<const float4 *>(gamma + c0 + 4 * q);
            const float4 be = *reinterpret_cast<const float4 *>(beta + c0 + 4 * q);
            const float mean = stat[p][0], rstd = stat[p][1];
            tile[4 * q + 0][p] = fmaf((v.x - mean) * rstd, g.x, be.x);
            tile[4 * q + 1][p] = fmaf((v.y - mean) * rstd, g.y, be.y);
            tile[4 * q + 2][p] = fmaf((v.z - mean) * rstd, g.z, be.z);
            tile[4 * q + 3][p] = fmaf((v.w - mean) * rstd, g.w, be.w);
        }
        __syncthreads();
        for (int ch = wave; ch < nc; ch += kFnThreads / 64)
            if (lane < np) out[((int64_t)n * c + c0 + ch) * hw + p0 + lane] = tile[ch][lane];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kFnThreads) focal_cast_kernel(const float *x, int64_t quads, uint16_t *out)
{
    const int64_t stride = (int64_t)gridDim.x * kFnThreads;
    for (int64_t i = (int64_t)blockIdx.x * kFnThreads + threadIdx.x; i < quads; i += stride) {
        const float4 v = *reinterpret_cast<const float4 *>(x + 4 * i);
        *reinterpret_cast<uint2 *>(out + 4 * i) = make_uint2(pack_act2(v.x, v.y), pack_act2(v.z, v.w));
    }
}

// ------------------------------------------------------------------------------------------------------------ host
int tiles_of(int h, int w) { return ((h + kFnTH - 1) / kFnTH) * ((w + kFnTW - 1) / kFnTW); }
int64_t sums_bytes(const sdetr_focalnet_op &o) { return (int64_t)o.batch * tiles_of(o.height, o.width) * o.in_channels * 4; }
int64_t finish_bytes(const sdetr_focalnet_op &o) { return sums_bytes(o) + (int64_t)o.batch * o.in_channels * 4; }

// kinds 3 .. 7 work on rows of C = in_channels, a multiple of 32
int check_rows(const char *what, const sdetr_focalnet_op &o, int precision)
{
    if (int rc = check_rows_shape(what, o.batch, o.height, o.width, o.in_channels, precision)) return rc;
    if (o.in_channels % 32 || o.in_channels > kRowMaxC)
        return fail("%s: channels must be a multiple of 32 up to %d (got %d)", what, kRowMaxC, o.in_channels);
    return 0;
}

// a GEMM op (kinds 0 .. 2) as the conv kernel's arguments
int make_gemm(const sdetr_focalnet_op &o, int precision, BConv &c)
{
    const char *what = "sdetr_focalnet (GEMM)";
    if (int rc = check_rows_shape(what, o.batch, o.height, o.width, o.in_channels, precision)) return rc;
    if (!o.x || !o.weight || !o.bias || !o.out) return fail("%s: null tensor", what);
    if (o.out_channels < 1) return fail("%s: bad out_channels %d", what, o.out_channels);
    if (o.kernel_size < 1 || o.kernel_size > 7 || o.stride < 1 || o.stride > 4 || o.padding < 0 || o.padding >= o.kernel_size)
        return fail("%s: kernel 1 .. 7, stride 1 .. 4, padding below the kernel (got kernel %d, stride %d, padding %d)", what,
                    o.kernel_size, o.stride, o.padding);
    if (o.x_nchw == 0 && o.in_channels % 32)
        return fail("%s: a channels-last input needs in_channels %% 32 == 0 (got %d)", what, o.in_channels);
    // the output size is the op's own: at least the unpadded convolution's, at most one more window of zero padding
    const int ho_min = out_hw(o.height, o.kernel_size, o.stride, o.padding), wo_min = out_hw(o.width, o.kernel_size, o.stride, o.padding);
    if (o.out_height < 1 || o.out_width < 1 || o.out_height < ho_min || o.out_width < wo_min ||
        (o.out_height - 1) * o.stride - o.padding >= o.height || (o.out_width - 1) * o.stride - o.padding >= o.width)
        return fail("%s: output %d x %d does not fit a %d x %d input (kernel %d, stride %d, padding %d)", what, o.out_height,
                    o.out_width, o.height, o.width, o.kernel_size, o.stride, o.padding);
    if (o.kind != 0 && (o.residual || o.x_nchw)) return fail("%s: only the linear epilogue takes a residual / the NCHW canvas", what);
    if (o.kind == 2 && (!o.q || o.q_ld < o.out_channels || o.q_ld % 4))
        return fail("%s: the product epilogue needs q with q_ld >= out_channels, q_ld %% 4 == 0", what);
    if (!all_aligned16(o.x, o.weight, o.out, o.bias, o.residual) || (o.kind == 2 && !aligned16(o.q)))
        return fail("%s: tensors must be 16-byte aligned", what);
    const ConvGeom g = {o.x, o.weight, o.bias, o.residual, o.out, o.batch, o.in_channels, o.height, o.width, o.out_channels,
                        o.kernel_size, o.stride, o.padding, o.out_height, o.out_width, o.x_nchw, o.splits};
    if (int rc = fill_conv(what, g, precision, c)) return rc;
    c.q = o.q;
    c.ldq = o.q_ld;
    return 0;
}

int run_gemm(hipStream_t s, const sdetr_focalnet_op &o, int precision, void *ws, int64_t ws_bytes)
{
    BConv c;
    if (int rc = make_gemm(o, precision, c)) return rc;
    if (conv_workspace(c) > ws_bytes || (conv_workspace(c) && !ws))
        return fail("sdetr_focalnet (GEMM): workspace of %lld bytes is too small (%lld needed)", (long long)ws_bytes,
                    (long long)conv_workspace(c));
    c.partial = reinterpret_cast<float *>(ws);
    const bool x3 = precision == 0;
    if (o.kind == 1) launch_rows_gemm<1>(s, c, x3);
    else if (o.kind == 2 && o.out_f32) launch_rows_gemm<4>(s, c, x3);
    else if (o.kind == 2) launch_rows_gemm<3>(s, c, x3);
    else launch_gemm<2>(s, c, x3, o.x_nchw != 0);
    return check_launch("sdetr_focalnet (GEMM)");
}

int make_level(const sdetr_focalnet_op &o, int precision, FnLevel &a)
{
    const char *what = "sdetr_focalnet (focal level)";
    if (int rc = check_rows(what, o, precision)) return rc;
    if (!o.x || !o.weight || !o.q || !o.out2) return fail("%s: null tensor", what);
    if (o.kernel_size != 3 && o.kernel_size != 5 && o.kernel_size != 7 && o.kernel_size != 9)
        return fail("%s: kernel size must be 3, 5, 7 or 9 (got %d)", what, o.kernel_size);
    if (o.x_ld < o.in_channels || o.x_ld % 4 || o.q_ld < 1) return fail("%s: bad row strides (x_ld %d, q_ld %d)", what, o.x_ld, o.q_ld);
    if (!all_aligned16(o.x, o.weight, o.out, o.out2) || (reinterpret_cast<uintptr_t>(o.q) & 3))
        return fail("%s: tensors must be 16-byte aligned", what);
    if ((int64_t)o.batch * o.height * o.width * o.x_ld >= (int64_t(1) << 31)) return fail("%s: tensors too large", what);
    a.x = reinterpret_cast<const float *>(o.x);
    a.taps = reinterpret_cast<const float *>(o.weight);
    a.gate = o.q;
    a.ctx = reinterpret_cast<float *>(o.out);
    a.all = reinterpret_cast<float *>(o.out2);
    a.sums = nullptr;
    a.x_ld = o.x_ld;
    a.gate_ld = o.q_ld;
    a.batch = o.batch;
    a.h = o.height;
    a.w = o.width;
    a.c = o.in_channels;
    a.tiles_x = (o.width + kFnTW - 1) / kFnTW;
    a.tiles_y = (o.height + kFnTH - 1) / kFnTH;
    a.accumulate = o.accumulate != 0;
    if (o.batch > 65535) return fail("%s: batch above 65535", what);
    return 0;
}

template <int K>
void launch_level(hipStream_t s, const FnLevel &a)
{
    constexpr int bytes = ((kFnTH + K - 1) * (kFnTW + K - 1) + K * K) * kFnCC * 4;   // 59 520 at K = 9
    static_assert(bytes <= 64 * 1024, "the focal level's tile fits the default LDS limit");
    hipLaunchKernelGGL(focal_level_kernel<K>, dim3((unsigned)(a.tiles_x * a.tiles_y), (unsigned)(a.c / kFnCC), (unsigned)a.batch),
                       dim3(kFnThreads), bytes, s, a);
}

int run_level(hipStream_t s, const sdetr_focalnet_op &o, int precision, void *ws, int64_t ws_bytes)
{
    FnLevel a;
    if (int rc = make_level(o, precision, a)) return rc;
    if (o.last) {
        if (!ws || ws_bytes < sums_bytes(o))
            return fail("sdetr_focalnet (focal level): workspace of %lld bytes is too small (%lld needed)", (long long)ws_bytes,
                        (long long)sums_bytes(o));
        a.sums = reinterpret_cast<float *>(ws);
    }
    if (o.kernel_size == 3) launch_level<3>(s, a);
    else if (o.kernel_size == 5) launch_level<5>(s, a);
    else if (o.kernel_size == 7) launch_level<7>(s, a);
    else launch_level<9>(s, a);
    return check_launch("sdetr_focalnet (focal level)");
}

int check_finish(const sdetr_focalnet_op &o, int precision)
{
    const char *what = "sdetr_focalnet (modulator finish)";
    if (int rc = check_rows(what, o, precision)) return rc;
    if (!o.x || !o.q || !o.out) return fail("%s: null tensor", what);
    if (o.q_ld < 1) return fail("%s: bad q_ld %d", what, o.q_ld);
    if (!all_aligned16(o.x, o.out) || (reinterpret_cast<uintptr_t>(o.q) & 3))
        return fail("%s: tensors must be 16-byte aligned", what);
    if (o.batch > 65535) return fail("%s: batch above 65535", what);
    return 0;
}

int run_finish(hipStream_t s, const sdetr_focalnet_op &o, int precision, void *ws, int64_t ws_bytes)
{
    if (int rc = check_finish(o, precision)) return rc;
    if (!ws || ws_bytes < finish_bytes(o))
        return fail("sdetr_focalnet (modulator finish): workspace of %lld bytes is too small (%lld needed)", (long long)ws_bytes,
                    (long long)finish_bytes(o));
    const int c = o.in_channels, hw = o.height * o.width, tiles = tiles_of(o.height, o.width);
    const float *sums = reinterpret_cast<const float *>(ws);
    float *mean = reinterpret_cast<float *>(reinterpret_cast<char *>(ws) + sums_bytes(o));
    hipLaunchKernelGGL(focal_mean_kernel, dim3((unsigned)((c + kFnThreads - 1) / kFnThreads), (unsigned)o.batch),
                       dim3(kFnThreads), 0, s, sums, tiles, c, 1.f / (float)hw, mean);
    const int64_t rows = (int64_t)o.batch * hw;
    const unsigned blocks = (unsigned)std::min<int64_t>((rows * (c / 4) + kFnThreads - 1) / kFnThreads, 16384);
    const float *all = reinterpret_cast<const float *>(o.x);
    if (precision == 0)
        hipLaunchKernelGGL(focal_finish_kernel<true>, dim3(blocks), dim3(kFnThreads), 0, s, all, mean, o.q, (int64_t)o.q_ld, rows,
                           hw, c, reinterpret_cast<char *>(o.out));
    else
        hipLaunchKernelGGL(focal_finish_kernel<false>, dim3(blocks), dim3(kFnThreads), 0, s, all, mean, o.q, (int64_t)o.q_ld, rows,
                           hw, c, reinterpret_cast<char *>(o.out));
    return check_launch("sdetr_focalnet (modulator finish)");
}

int check_ln(const sdetr_focalnet_op &o, int precision)
{
    const char *what = "sdetr_focalnet (LayerNorm)";
    if (int rc = check_ln_rows(what, o.batch, o.height, o.width, o.in_channels, precision, o.x, o.gamma, o.beta, o.out)) return rc;
    if (o.kind == 6 && (o.residual || o.out2)) return fail("%s: the NCHW form takes no residual / 16-bit copy", what);
    if (o.out2 && precision == 0) return fail("%s: the 16-bit copy exists in 16-bit mode only", what);
    if (!all_aligned16(o.residual, o.out2)) return fail("%s: tensors must be 16-byte aligned", what);
    if (o.batch > 65535) return fail("%s: batch above 65535", what);
    return 0;
}

int run_ln(hipStream_t s, const sdetr_focalnet_op &o, int precision)
{
    if (int rc = check_ln(o, precision)) return rc;
    const int hw = o.height * o.width;
    if (o.kind == 6)
        hipLaunchKernelGGL(focal_ln_nchw_kernel, dim3((unsigned)((hw + 63) / 64), (unsigned)o.batch), dim3(kFnThreads), 0, s,
                           reinterpret_cast<const float *>(o.x), o.gamma, o.beta, hw, o.in_channels, o.eps,
                           reinterpret_cast<float *>(o.out));
    else
        launch_ln_rows(s, precision == 0 || o.out_f32, o.x, o.gamma, o.beta, o.residual, (int64_t)o.batch * hw, o.in_channels,
                       o.eps, o.out, o.out2);
    return check_launch("sdetr_focalnet (LayerNorm)");
}

int check_cast(const sdetr_focalnet_op &o, int precision)
{
    const char *what = "sdetr_focalnet (cast)";
    if (int rc = check_rows(what, o, precision)) return rc;
    if (precision != 1) return fail("%s: 16-bit mode only", what);
    if (!o.x || !o.out) return fail("%s: null tensor", what);
    if (!all_aligned16(o.x, o.out)) return fail("%s: tensors must be 16-byte aligned", what);
    return 0;
}

int run_cast(hipStream_t s, const sdetr_focalnet_op &o, int precision)
{
    if (int rc = check_cast(o, precision)) return rc;
    const int64_t quads = (int64_t)o.batch * o.height * o.width * (o.in_channels / 4);
    const unsigned blocks = (unsigned)std::min<int64_t>((quads + kFnThreads - 1) / kFnThreads, 16384);
    hipLaunchKernelGGL(focal_cast_kernel, dim3(blocks), dim3(kFnThreads), 0, s, reinterpret_cast<const float *>(o.x), quads,
                       reinterpret_cast<uint16_t *>(o.out));
    return check_launch("sdetr_focalnet (cast)");
}

// validation of one op without a launch; `need` receives its workspace bytes
int check_op(const sdetr_focalnet_op &o, int precision, int64_t &need)
{
    need = 0;
    if (o.kind >= 0 && o.kind <= 2) {
        BConv c;
        if (int rc = make_gemm(o, precision, c)) return rc;
        need = conv_workspace(c);
        return 0;
    }
    if (o.kind == 3) {
        FnLevel a;
        if (int rc = make_level(o, precision, a)) return rc;
        need = o.last ? sums_bytes(o) : 0;
        return 0;
    }
    if (o.kind == 4) {
        if (int rc = check_finish(o, precision)) return rc;
        need = finish_bytes(o);
        return 0;
    }
    if (o.kind == 5 || o.kind == 6) return check_ln(o, precision);
    if (o.kind == 7) return check_cast(o, precision);
    return fail("sdetr_focalnet: unknown op kind %d", o.kind);
}

int run_op(hipStream_t s, const sdetr_focalnet_op &o, int precision, void *ws, int64_t ws_bytes)
{
    if (o.kind >= 0 && o.kind <= 2) return run_gemm(s, o, precision, ws, ws_bytes);
    if (o.kind == 3) return run_level(s, o, precision, ws, ws_bytes);
    if (o.kind == 4) return run_finish(s, o, precision, ws, ws_bytes);
    if (o.kind == 5 || o.kind == 6) return run_ln(s, o, precision);
    if (o.kind == 7) return run_cast(s, o, precision);
    return fail("sdetr_focalnet: unknown op kind %d", o.kind);
}

}  // namespace
}  // namespace sdetr

using namespace sdetr;

using FocalnetPlan = Plan<sdetr_focalnet_op, check_op, run_op>;

extern "C" int64_t sdetr_focalnet_workspace_bytes(const sdetr_focalnet_op *ops, int n_ops, int precision)
{
    return FocalnetPlan::workspace_bytes(ops, n_ops, precision);
}

extern "C" int sdetr_focalnet_op_run(sdetr_stream_t stream, const sdetr_focalnet_op *op, int precision, void *workspace,
                                     int64_t workspace_bytes)
{
    return FocalnetPlan::op_run("sdetr_focalnet", stream, op, precision, workspace, workspace_bytes);
}

extern "C" int sdetr_focalnet_run(sdetr_stream_t stream, const sdetr_focalnet_op *ops, int n_ops, int precision,
                                  void *workspace, int64_t workspace_bytes)
{
    return FocalnetPlan::run("sdetr_focalnet", stream, ops, n_ops, precision, workspace, workspace_bytes);
}

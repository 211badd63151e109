// The ChannelMapper's backward (training; frontend.hip is the forward and holds the training forward's GroupNorm launch,
// sdetr_frontend_groupnorm_train, next to the kernel it shares with inference).  A level is y = GroupNorm(conv(x)): its
// backward is the GroupNorm backward here, then the backbone's backward-weight and backward-data kernels on the result
// (sdetr_backbone_wgrad / _dgrad, backbone_backward.hip; nothing of them is repeated here), whose operands are
// channels-last in the compute dtype.  The maps on either side of the mapper are fp32 NCHW, so the kernels of this file turn
// the layout on the way: a tile of 32 channels x 128 pixels goes through LDS, rows 129 words apart (the channels-last side
// touches 32 rows at one pixel, the NCHW side one row at 64 pixels: both conflict-free).
//   fgb_partial_kernel   per (image, channel, 128-pixel tile): sum of (dy + add) and of (dy + add) * xh, xh = (z - mean) * rstd
//   fgb_finish_kernel    a workgroup per group: the tiles in tile order -> per-(image, channel) sums; dgamma / dbeta over the
//                        images in image order; the group's two means (gamma-weighted, in channel order)
//   fgb_apply_kernel     dz = rstd * (g - mean(g) - xh * mean(g * xh)), g = gamma * (dy + add), written channels-last
//   fgb_egest_kernel     channels-last (+ a second one) -> fp32 NCHW
// No atomics: every sum has a fixed order.  Every launch writes every element of its outputs.
#include "backbone_rows_core.h"

namespace sdetr {
namespace {

constexpr int kGbThreads = 256;
constexpr int kGbCh = 32;                   // channels per tile
constexpr int kGbPx = 128;                  // pixels per tile: the unit of the first pass's partial sums
constexpr int kGbRow = kGbPx + 1;           // words per LDS row

struct GbArgs {
    const float *dy;        // [B, C, P]
    const char *add;        // [B, P, C] compute dtype, or null
    const float *z;         // [B, C, P]
    const float *stats;     // [B][G][2] (mean, rstd)
    const float *gamma;     // [C]
    char *out;              // [B, P, C] compute dtype
    float *dgamma, *dbeta;  // [C], or both null
    float *part;            // [B][C][tiles][2]
    float *sums;            // [B][C][2]
    float *coef;            // [B][G][2]: mean_group(g), mean_group(g * xh)
    int batch, c, p, groups, tiles;
};

// four consecutive channels of a channels-last row at element e (channel ch of C); zeros past C.  `vec`: C % 4 == 0
template <bool X3>
__device__ __forceinline__ float4 cl_load4(const char *base, int64_t e, int ch, int C, bool vec)
{
    if (vec) {
        if (ch >= C) return make_float4(0.f, 0.f, 0.f, 0.f);
        if (X3) return *reinterpret_cast<const float4 *>(base + e * 4);
        const uint2 v = *reinterpret_cast<const uint2 *>(base + e * 2);
        return make_float4(act_lo(v.x), act_hi(v.x), act_lo(v.y), act_hi(v.y));
    }
    float r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r[i] = 0.f;
        if (ch + i < C)
            r[i] = X3 ? reinterpret_cast<const float *>(base)[e + i] : act_lo(reinterpret_cast<const uint16_t *>(base)[e + i]);
    }
    return make_float4(r[0], r[1], r[2], r[3]);
}

template <bool X3>
__device__ __forceinline__ void cl_store4(char *base, int64_t e, int ch, int C, bool vec, float4 v)
{
    if (vec) {
        if (ch >= C) return;
        if (X3) *reinterpret_cast<float4 *>(base + e * 4) = v;
        else *reinterpret_cast<uint2 *>(base + e * 2) = make_uint2(pack_act2(v.x, v.y), pack_act2(v.z, v.w));
        return;
    }
    const float r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (ch + i >= C) continue;
        if (X3) reinterpret_cast<float *>(base)[e + i] = r[i];
        else reinterpret_cast<uint16_t *>(base)[e + i] = (uint16_t)(pack_act2(r[i], 0.f) & 0xffffu);
    }
}

// channels-last tile (pixels p0 .., channels c0 ..) of image n (+ a second tensor) -> tile[channel][pixel]; a thread takes
// four channels of one pixel
template <bool X3>
__device__ __forceinline__ void cl_tile_load(const char *a, const char *b, int n, int p0, int c0, int P, int C, float *tile)
{
    const int q = threadIdx.x & 7, ch = c0 + 4 * q;
    const bool vec = (C & 3) == 0;
#pragma unroll
    for (int r = 0; r < kGbPx / 32; ++r) {
        const int px = (threadIdx.x >> 3) + 32 * r, p = p0 + px;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p < P) {
            const int64_t e = ((int64_t)n * P + p) * C + ch;
            v = cl_load4<X3>(a, e, ch, C, vec);
            if (b) {
                const float4 w = cl_load4<X3>(b, e, ch, C, vec);
                v.x += w.x, v.y += w.y, v.z += w.z, v.w += w.w;
            }
        }
        tile[(4 * q) * kGbRow + px] = v.x;
        tile[(4 * q + 1) * kGbRow + px] = v.y;
        tile[(4 * q + 2) * kGbRow + px] = v.z;
        tile[(4 * q + 3) * kGbRow + px] = v.w;
    }
}

template <bool X3>
__device__ __forceinline__ void cl_tile_store(char *out, int n, int p0, int c0, int P, int C, const float *tile)
{
    const int q = threadIdx.x & 7, ch = c0 + 4 * q;
    const bool vec = (C & 3) == 0;
#pragma unroll
    for (int r = 0; r < kGbPx / 32; ++r) {
        const int px = (threadIdx.x >> 3) + 32 * r, p = p0 + px;
        if (p >= P) continue;
        const float4 v = make_float4(tile[(4 * q) * kGbRow + px], tile[(4 * q + 1) * kGbRow + px], tile[(4 * q + 2) * kGbRow + px],
                                     tile[(4 * q + 3) * kGbRow + px]);
        cl_store4<X3>(out, ((int64_t)n * P + p) * C + ch, ch, C, vec, v);
    }
}

// grid (tiles, channel tiles, batch).  A wave takes channels wave, wave + 4, ..; a lane pixels lane and lane + 64.
// APPLY false: the first pass (the tile's two sums per channel); true: the element-wise pass
template <bool X3, bool APPLY>
__global__ void __launch_bounds__(kGbThreads) fgb_tile_kernel(GbArgs a)
{
    __shared__ float tile[kGbCh * kGbRow];
    const int t = blockIdx.x, c0 = blockIdx.y * kGbCh, n = blockIdx.z, p0 = t * kGbPx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cg = a.c / a.groups;
    if (a.add) {
        cl_tile_load<X3>(a.add, nullptr, n, p0, c0, a.p, a.c, tile);
        __syncthreads();
    }
    const float inv = 1.f / ((float)cg * (float)a.p);
    for (int i = wave; i < kGbCh; i += kGbThreads / 64) {
        const int c = c0 + i;
        if (c >= a.c) break;                                   // (uniform over the wave)
        const int g = c / cg;
        const float mean = a.stats[((int64_t)n * a.groups + g) * 2], rstd = a.stats[((int64_t)n * a.groups + g) * 2 + 1];
        const float *dy = a.dy + ((int64_t)n * a.c + c) * a.p, *z = a.z + ((int64_t)n * a.c + c) * a.p;
        float gam = 0.f, m1 = 0.f, m2 = 0.f, s1 = 0.f, s2 = 0.f;
        if (APPLY) {
            gam = a.gamma[c];
            m1 = a.coef[((int64_t)n * a.groups + g) * 2] * inv;
            m2 = a.coef[((int64_t)n * a.groups + g) * 2 + 1] * inv;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int px = lane + 64 * h, p = p0 + px;
            if (p >= a.p) continue;
            float v = dy[p];
            if (a.add) v += tile[i * kGbRow + px];
            const float xh = (z[p] - mean) * rstd;
            if (APPLY) {
                tile[i * kGbRow + px] = rstd * (gam * v - m1 - xh * m2);
            } else {
                s1 += v;
                s2 += v * xh;
            }
        }
        if (!APPLY) {
            s1 = wave_sum(s1);
            s2 = wave_sum(s2);
            if (lane == 0) {
                float *pt = a.part + (((int64_t)n * a.c + c) * a.tiles + t) * 2;
                pt[0] = s1;
                pt[1] = s2;
            }
        }
    }
    if (!APPLY) return;
    __syncthreads();
    cl_tile_store<X3>(a.out, n, p0, c0, a.p, a.c, tile);
}

// grid (groups): the tiles of every (image, channel) of the group in tile order; then dgamma / dbeta over the images in
// image order and the group's gamma-weighted sums in channel order
__global__ void __launch_bounds__(kGbThreads) fgb_finish_kernel(GbArgs a)
{
    const int g = blockIdx.x, cg = a.c / a.groups, tid = threadIdx.x;
    for (int i = tid; i < a.batch * cg; i += kGbThreads) {
        const int n = i / cg, c = g * cg + (i - n * cg);
        const float *pt = a.part + ((int64_t)n * a.c + c) * a.tiles * 2;
        float s1 = 0.f, s2 = 0.f;
        for (int t = 0; t < a.tiles; ++t) {
            s1 += pt[2 * t];
            s2 += pt[2 * t + 1];
        }
        a.sums[((int64_t)n * a.c + c) * 2] = s1;
        a.sums[((int64_t)n * a.c + c) * 2 + 1] = s2;
    }
    __syncthreads();                                            // (this workgroup's own writes to sums are visible to it)
    if (a.dgamma)
        for (int j = tid; j < cg; j += kGbThreads) {
            const int c = g * cg + j;
            float s1 = 0.f, s2 = 0.f;
            for (int n = 0; n < a.batch; ++n) {
                s1 += a.sums[((int64_t)n * a.c + c) * 2];
                s2 += a.sums[((int64_t)n * a.c + c) * 2 + 1];
            }
            a.dbeta[c] = s1;
            a.dgamma[c] = s2;
        }
    for (int n = tid; n < a.batch; n += kGbThreads) {
        float m1 = 0.f, m2 = 0.f;
        for (int j = 0; j < cg; ++j) {
            const int c = g * cg + j;
            const float gam = a.gamma[c];
            m1 += gam * a.sums[((int64_t)n * a.c + c) * 2];
            m2 += gam * a.sums[((int64_t)n * a.c + c) * 2 + 1];
        }
        a.coef[((int64_t)n * a.groups + g) * 2] = m1;
        a.coef[((int64_t)n * a.groups + g) * 2 + 1] = m2;
    }
}

// grid (tiles, channel tiles, batch): a [B, P, C] (+ b) compute dtype -> out f32 [B, C, P]
template <bool X3>
__global__ void __launch_bounds__(kGbThreads) fgb_egest_kernel(const char *a, const char *b, int C, int P, float *out)
{
    __shared__ float tile[kGbCh * kGbRow];
    const int c0 = blockIdx.y * kGbCh, n = blockIdx.z, p0 = blockIdx.x * kGbPx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    cl_tile_load<X3>(a, b, n, p0, c0, P, C, tile);
    __syncthreads();
    for (int i = wave; i < kGbCh; i += kGbThreads / 64) {
        const int c = c0 + i;
        if (c >= C) break;
        float *dst = out + ((int64_t)n * C + c) * P;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int px = lane + 64 * h;
            if (p0 + px < P) dst[p0 + px] = tile[i * kGbRow + px];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------ host
const char *kind_name(int kind)
{
    static const char *names[] = {"dgrad", "wgrad", "rows", "group norm", "egest"};
    return kind >= 0 && kind <= 4 ? names[kind] : "?";
}

// kinds 0 .. 2 as the backbone backward's op
sdetr_backbone_bwd_op conv_op(const sdetr_frontend_bwd_op &o)
{
    sdetr_backbone_bwd_op b = {};
    b.kind = o.kind;
    b.dz = o.kind == 2 ? o.x : o.dz;
    b.x = o.x;
    b.weight = o.weight;
    b.scale = o.scale;
    b.add = o.add;
    b.out = o.out;
    b.batch = o.batch;
    b.in_channels = o.in_channels;
    b.height = o.height;
    b.width = o.width;
    b.out_channels = o.out_channels;
    b.kernel_size = o.kernel_size;
    b.stride = o.kernel_size == 3 ? 2 : 1;
    b.padding = (o.kernel_size - 1) / 2;
    b.splits = o.splits;
    return b;
}

inline int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

struct GbPlan {
    int tiles;
    int64_t off_sums, off_coef, need;
};

// the grid of a tile kernel over [batch, channels, pixels]
int check_tiles(const char *what, int batch, int channels, int64_t pixels)
{
    if (batch > 65535 || (channels + kGbCh - 1) / kGbCh > 65535 || pixels >= (int64_t(1) << 30))
        return fail("%s: too many images, channels or pixels for one launch", what);
    return 0;
}

int check_groupnorm(const sdetr_frontend_bwd_op &o, int precision, GbPlan &p)
{
    const char *what = "sdetr_frontend_bwd (group norm)";
    if (int rc = check_rows_shape(what, o.batch, o.height, o.width, o.out_channels, precision)) return rc;
    if (o.groups < 1 || o.out_channels % o.groups)
        return fail("%s: %d channels in %d groups", what, o.out_channels, o.groups);
    if (!(o.eps >= 0.f)) return fail("%s: bad eps %g", what, (double)o.eps);
    if (!o.dz || !o.z || !o.stats || !o.gamma || !o.out || (!o.dgamma != !o.dbeta))
        return fail("%s: null tensor (dgamma and dbeta go together)", what);
    if (!all_aligned16(o.dz, o.z, o.stats, o.gamma, o.out, o.add, o.dgamma, o.dbeta))
        return fail("%s: tensors must be 16-byte aligned", what);
    if (o.out == o.add) return fail("%s: out must not alias add", what);
    const int64_t pixels = (int64_t)o.height * o.width;
    if (int rc = check_tiles(what, o.batch, o.out_channels, pixels)) return rc;
    p.tiles = (int)((pixels + kGbPx - 1) / kGbPx);
    p.off_sums = align256((int64_t)o.batch * o.out_channels * p.tiles * 2 * 4);
    p.off_coef = p.off_sums + align256((int64_t)o.batch * o.out_channels * 2 * 4);
    p.need = p.off_coef + align256((int64_t)o.batch * o.groups * 2 * 4);
    return 0;
}

int check_egest(const sdetr_frontend_bwd_op &o, int precision)
{
    const char *what = "sdetr_frontend_bwd (egest)";
    if (int rc = check_rows_shape(what, o.batch, o.height, o.width, o.in_channels, precision)) return rc;
    if (!o.dz || !o.out) return fail("%s: null tensor", what);
    if (!all_aligned16(o.dz, o.add, o.out)) return fail("%s: tensors must be 16-byte aligned", what);
    return check_tiles(what, o.batch, o.in_channels, (int64_t)o.height * o.width);
}

// validation of one op without a launch
int check_op(const sdetr_frontend_bwd_op &o, int precision, GbPlan &p)
{
    p = GbPlan{};
    if (o.kind < 0 || o.kind > 4) return fail("sdetr_frontend_bwd: unknown op kind %d", o.kind);
    if (precision != 0 && precision != 1) return fail("sdetr_frontend_bwd (%s): precision must be 0 or 1", kind_name(o.kind));
    if (o.kind <= 2) {
        if (o.kind != 2 && o.kernel_size != 1 && o.kernel_size != 3)
            return fail("sdetr_frontend_bwd (%s): kernel_size %d (1 or 3)", kind_name(o.kind), o.kernel_size);
        const sdetr_backbone_bwd_op b = conv_op(o);
        p.need = sdetr_backbone_bwd_workspace_bytes(&b, 1, precision);
        return p.need < 0 ? SDETR_EINVAL : 0;
    }
    if (o.kind == 3) return check_groupnorm(o, precision, p);
    return check_egest(o, precision);
}

int check_bwd_op(const sdetr_frontend_bwd_op &o, int precision, int64_t &need)
{
    GbPlan p;
    const int rc = check_op(o, precision, p);
    need = rc ? 0 : p.need;
    return rc;
}

int run_bwd_op(hipStream_t s, const sdetr_frontend_bwd_op &o, int precision, void *ws, int64_t ws_bytes)
{
    GbPlan p;
    if (int rc = check_op(o, precision, p)) return rc;
    if (p.need > ws_bytes || (p.need && !ws))
        return fail("sdetr_frontend_bwd (%s): workspace of %lld bytes is too small (%lld needed)", kind_name(o.kind),
                    (long long)ws_bytes, (long long)p.need);
    if (o.kind <= 2) {
        const sdetr_backbone_bwd_op b = conv_op(o);
        if (o.kind == 0) return sdetr_backbone_dgrad((sdetr_stream_t)s, &b, precision, ws, ws_bytes);
        if (o.kind == 1) return sdetr_backbone_wgrad((sdetr_stream_t)s, &b, precision, ws, ws_bytes);
        return sdetr_backbone_bwd_run((sdetr_stream_t)s, &b, 1, precision, ws, ws_bytes);
    }
    const int P = o.height * o.width;
    if (o.kind == 3) {
        char *w = reinterpret_cast<char *>(ws);
        GbArgs a;
        a.dy = reinterpret_cast<const float *>(o.dz);
        a.add = reinterpret_cast<const char *>(o.add);
        a.z = o.z;
        a.stats = o.stats;
        a.gamma = o.gamma;
        a.out = reinterpret_cast<char *>(o.out);
        a.dgamma = o.dgamma;
        a.dbeta = o.dbeta;
        a.part = reinterpret_cast<float *>(w);
        a.sums = reinterpret_cast<float *>(w + p.off_sums);
        a.coef = reinterpret_cast<float *>(w + p.off_coef);
        a.batch = o.batch;
        a.c = o.out_channels;
        a.p = P;
        a.groups = o.groups;
        a.tiles = p.tiles;
        const dim3 grid((unsigned)p.tiles, (unsigned)((a.c + kGbCh - 1) / kGbCh), (unsigned)o.batch);
        if (precision == 0) hipLaunchKernelGGL((fgb_tile_kernel<true, false>), grid, dim3(kGbThreads), 0, s, a);
        else hipLaunchKernelGGL((fgb_tile_kernel<false, false>), grid, dim3(kGbThreads), 0, s, a);
        hipLaunchKernelGGL(fgb_finish_kernel, dim3((unsigned)o.groups), dim3(kGbThreads), 0, s, a);
        if (precision == 0) hipLaunchKernelGGL((fgb_tile_kernel<true, true>), grid, dim3(kGbThreads), 0, s, a);
        else hipLaunchKernelGGL((fgb_tile_kernel<false, true>), grid, dim3(kGbThreads), 0, s, a);
    } else {
        const dim3 grid((unsigned)((P + kGbPx - 1) / kGbPx), (unsigned)((o.in_channels + kGbCh - 1) / kGbCh), (unsigned)o.batch);
        const char *a = reinterpret_cast<const char *>(o.dz), *b = reinterpret_cast<const char *>(o.add);
        float *out = reinterpret_cast<float *>(o.out);
        if (precision == 0) hipLaunchKernelGGL(fgb_egest_kernel<true>, grid, dim3(kGbThreads), 0, s, a, b, o.in_channels, P, out);
        else hipLaunchKernelGGL(fgb_egest_kernel<false>, grid, dim3(kGbThreads), 0, s, a, b, o.in_channels, P, out);
    }
    return check_launch("sdetr_frontend_bwd");
}

}  // namespace
}  // namespace sdetr

using namespace sdetr;

using FrontendBwdPlan = Plan<sdetr_frontend_bwd_op, check_bwd_op, run_bwd_op>;

extern "C" int64_t sdetr_frontend_bwd_workspace_bytes(const sdetr_frontend_bwd_op *ops, int n_ops, int precision)
{
    return FrontendBwdPlan::workspace_bytes(ops, n_ops, precision);
}

extern "C" int sdetr_frontend_bwd_op_run(sdetr_stream_t stream, const sdetr_frontend_bwd_op *op, int precision, void *workspace,
                                         int64_t workspace_bytes)
{
    return FrontendBwdPlan::op_run("sdetr_frontend_bwd", stream, op, precision, workspace, workspace_bytes);
}

extern "C" int sdetr_frontend_bwd_run(sdetr_stream_t stream, const sdetr_frontend_bwd_op *ops, int n_ops, int precision,
                                      void *workspace, int64_t workspace_bytes)
{
    return FrontendBwdPlan::run("sdetr_frontend_bwd", stream, ops, n_ops, precision, workspace, workspace_bytes);
}

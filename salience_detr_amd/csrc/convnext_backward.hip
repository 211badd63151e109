// The ConvNeXt backbone's backward (training; convnext.hip is the forward).  For a block
//   y = x + s[n] * g (.) (W2 gelu(W1 LN(dw(x) + bd) + b1) + b2)
// and a down-sampler Conv2d(k = 2, s = 2)(LayerNorm2d(y)).  The residual-stream gradient is channels-last fp32 in every
// precision; the GEMM operands are in the compute dtype.  The two Linears (and the down-sampler over its space-to-depth
// rows) go to backbone_backward.hip's backward-data and backward-weight kernels through their C entry points; here are
//   cnb_rows_kernel        s[n] * dy -> the compute dtype (MODE 2), or dh * gelu'(pre) (MODE 3), with the column sums (the
//                          bias gradients): lanes along C (one quad each), a workgroup's four waves walk a strip of rows,
//                          one partial [C] per strip
//   cnb_ln_kernel          LayerNorm backward over C: one wave per row, the row in registers, the statistics recomputed
//                          as the forward computes them; dgamma / dbeta accumulate per wave in LDS, one partial [2][C] per
//                          workgroup
//   cnb_dw_wgrad_kernel    depthwise 7x7 backward-weight: lanes along C, a wave owns a strip of (row, 32-pixel segment)
//                          units and holds its channel's 49 tap sums (+ the bias sum) in registers, a 7-wide window
//                          sliding along the input row; one partial [50][C] per strip
//   cnb_dw_dgrad_kernel    depthwise 7x7 backward-data (the taps reversed) + the identity branch, a 7 x 7 sliding window
//   cnb_sum_kernel         the partials of any of the above added in strip order
//   cnb_scale_kernel       layer scale: dW2 = g dW2', db2 = g db2', dg = <dW2', W2> + db2' b2 (no u = W2 h + b2 needed)
//   cnb_patches / _pixels  the down-sampler's space-to-depth rows and back (cropped pixels: exact zeros)
//   cnb_ingest_kernel      a returned map's fp32 NCHW cotangent (+ the gradient arriving from above) as fp32 rows
// No atomics: every sum has a fixed order.  Every launch writes every element of its outputs.
#include "backbone_rows_core.h"

namespace sdetr {
namespace {

constexpr int kCbThreads = 256;
constexpr int kCbSeg = 32;                    // pixels of one depthwise unit along x
constexpr int kCbMaxC = 3072;

template <bool X3>
__device__ __forceinline__ float4 load_quad(const char *p, int64_t e)
{
    if (X3) return *reinterpret_cast<const float4 *>(p + e * 4);
    const uint2 v = *reinterpret_cast<const uint2 *>(p + e * 2);
    return make_float4(act_lo(v.x), act_hi(v.x), act_lo(v.y), act_hi(v.y));
}
template <bool X3>
__device__ __forceinline__ void store_quad(char *p, int64_t e, float4 v)
{
    if (X3) *reinterpret_cast<float4 *>(p + e * 4) = v;
    else *reinterpret_cast<uint2 *>(p + e * 2) = make_uint2(pack_act2(v.x, v.y), pack_act2(v.z, v.w));
}

// d/dx of gelu_erf: Phi(x) + x phi(x), Phi through the forward's fitted erf
__device__ __forceinline__ float gelu_erf_grad(float x)
{
    const float e = erf_pos(fabsf(x) * 0.70710678118654752440f);
    const float cdf = 0.5f + copysignf(0.5f * e, x);
    const float pdf = 0.3989422804014327f * __expf(-0.5f * x * x);
    return fmaf(x, pdf, cdf);
}

struct CbRows {
    const char *dz, *x;
    const float *scale;
    char *out;
    float *partial;       // [strips][C]
    int64_t rows;
    int c, hw;
};

// MODE 2: out = scale[n] * dz (dz fp32); MODE 3: out = dz * gelu'(x) (dz, x compute dtype).  grid (strips, quad chunks)
template <bool X3, int MODE>
__global__ void __launch_bounds__(kCbThreads) cnb_rows_kernel(CbRows a)
{
    __shared__ float4 red[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.y * 64 + lane;
    const bool active = q < (a.c >> 2);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active) {
        const int64_t step = (int64_t)gridDim.x * 4;
        for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < a.rows; r += step) {
            const int64_t e = r * a.c + 4 * q;
            float4 v;
            if (MODE == 2) {
                v = *reinterpret_cast<const float4 *>(a.dz + e * 4);
                if (a.scale) {
                    const float s = a.scale[r / a.hw];
                    v.x *= s, v.y *= s, v.z *= s, v.w *= s;
                }
            } else {
                v = load_quad<X3>(a.dz, e);
                const float4 p = load_quad<X3>(a.x, e);
                v.x *= gelu_erf_grad(p.x), v.y *= gelu_erf_grad(p.y), v.z *= gelu_erf_grad(p.z), v.w *= gelu_erf_grad(p.w);
            }
            store_quad<X3>(a.out, e, v);
            acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
        }
    }
    red[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && active) {
        float4 s = red[0][lane];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            const float4 t = red[w][lane];
            s.x += t.x, s.y += t.y, s.z += t.z, s.w += t.w;
        }
        *reinterpret_cast<float4 *>(a.partial + (int64_t)blockIdx.x * a.c + 4 * q) = s;
    }
}

// out0[col] (col < split) / out1[col - split] = the partials [strips][cols] added in strip order; a null out is skipped
__global__ void __launch_bounds__(256) cnb_sum_kernel(const float *partial, int strips, int cols, int split, float *out0,
                                                      float *out1)
{
    const int col = blockIdx.x * 256 + threadIdx.x;
    if (col >= cols) return;
    float *dst = col < split ? (out0 ? out0 + col : nullptr) : (out1 ? out1 + (col - split) : nullptr);
    if (!dst) return;
    float v = partial[col];
    for (int s = 1; s < strips; ++s) v += partial[(int64_t)s * cols + col];
    *dst = v;
}

struct CbLn {
    const char *dz;       // [rows][C] compute dtype
    const float *x, *gamma, *add;
    float *out;
    float *partial;       // [blocks][2][C]
    int64_t rows;
    int c;
    float eps;
};

template <bool X3>
__global__ void __launch_bounds__(kCbThreads) cnb_ln_kernel(CbLn a)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nq = a.c >> 2;
    float *mine = reinterpret_cast<float *>(lds) + (int64_t)wave * 2 * a.c;   // [2][C]: dgamma, dbeta of this wave's rows
    for (int q = lane; q < 2 * nq; q += 64) *reinterpret_cast<float4 *>(mine + 4 * q) = make_float4(0.f, 0.f, 0.f, 0.f);
    const float inv_c = 1.f / (float)a.c;
    const int64_t step = (int64_t)gridDim.x * 4;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < a.rows; r += step) {
        LnRow row;
        ln_row_load(a.x + r * a.c, nq, lane, row);
        ln_row_stats(nq, lane, inv_c, a.eps, row);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < kRowQuads; ++i) {
            const int q = lane + 64 * i;
            if (q >= nq) continue;
            const float4 d = load_quad<X3>(a.dz, r * a.c + 4 * q);
            const float4 g = *reinterpret_cast<const float4 *>(a.gamma + 4 * q);
            const float g0 = d.x * g.x, g1 = d.y * g.y, g2 = d.z * g.z, g3 = d.w * g.w;
            s1 += (g0 + g1) + (g2 + g3);
            const float h0 = (row.v[i].x - row.mean) * row.rstd, h1 = (row.v[i].y - row.mean) * row.rstd;
            const float h2 = (row.v[i].z - row.mean) * row.rstd, h3 = (row.v[i].w - row.mean) * row.rstd;
            s2 += (g0 * h0 + g1 * h1) + (g2 * h2 + g3 * h3);
        }
        const float ma = wave_sum(s1) * inv_c, mb = wave_sum(s2) * inv_c;
#pragma unroll
        for (int i = 0; i < kRowQuads; ++i) {
            const int q = lane + 64 * i;
            if (q >= nq) continue;
            const int64_t e = r * a.c + 4 * q;
            const float4 d = load_quad<X3>(a.dz, e);
            const float4 g = *reinterpret_cast<const float4 *>(a.gamma + 4 * q);
            const float h0 = (row.v[i].x - row.mean) * row.rstd, h1 = (row.v[i].y - row.mean) * row.rstd;
            const float h2 = (row.v[i].z - row.mean) * row.rstd, h3 = (row.v[i].w - row.mean) * row.rstd;
            float4 o;
            o.x = row.rstd * (d.x * g.x - ma - h0 * mb);
            o.y = row.rstd * (d.y * g.y - ma - h1 * mb);
            o.z = row.rstd * (d.z * g.z - ma - h2 * mb);
            o.w = row.rstd * (d.w * g.w - ma - h3 * mb);
            if (a.add) {
                const float4 b = *reinterpret_cast<const float4 *>(a.add + e);
                o.x += b.x, o.y += b.y, o.z += b.z, o.w += b.w;
            }
            *reinterpret_cast<float4 *>(a.out + e) = o;
            float4 dg = *reinterpret_cast<float4 *>(mine + 4 * q), db = *reinterpret_cast<float4 *>(mine + a.c + 4 * q);
            dg.x = fmaf(d.x, h0, dg.x), dg.y = fmaf(d.y, h1, dg.y), dg.z = fmaf(d.z, h2, dg.z), dg.w = fmaf(d.w, h3, dg.w);
            db.x += d.x, db.y += d.y, db.z += d.z, db.w += d.w;
            *reinterpret_cast<float4 *>(mine + 4 * q) = dg;
            *reinterpret_cast<float4 *>(mine + a.c + 4 * q) = db;
        }
    }
    __syncthreads();
    const float *all = reinterpret_cast<const float *>(lds);
    for (int i = threadIdx.x; i < 2 * a.c; i += kCbThreads) {
        float v = all[i];
#pragma unroll
        for (int w = 1; w < 4; ++w) v += all[(int64_t)w * 2 * a.c + i];
        a.partial[(int64_t)blockIdx.x * 2 * a.c + i] = v;
    }
}

struct CbDw {
    const float *dz, *x, *taps, *add;
    float *out;
    float *partial;       // wgrad: [strips][50][C]
    int batch, h, w, c, nseg, units, strips;
};

// grid (ceil(strips / 4), ceil(C / 64)): wave `strip` walks the units strip, strip + strips, ..
__global__ void __launch_bounds__(kCbThreads) cnb_dw_wgrad_kernel(CbDw a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int strip = blockIdx.x * 4 + wave, c = blockIdx.y * 64 + lane;
    if (strip >= a.strips || c >= a.c) return;
    float acc[50];
#pragma unroll
    for (int t = 0; t < 50; ++t) acc[t] = 0.f;
    for (int u = strip; u < a.units; u += a.strips) {
        const int seg = u % a.nseg, rowi = u / a.nseg, y = rowi % a.h, n = rowi / a.h;
        const int x0 = seg * kCbSeg, x1 = min(a.w, x0 + kCbSeg);
        const float *dr = a.dz + ((int64_t)(n * a.h + y) * a.w) * a.c + c;
#pragma unroll
        for (int ky = 0; ky < 7; ++ky) {
            const int iy = y + ky - 3;
            if (iy < 0 || iy >= a.h) continue;
            const float *xr = a.x + ((int64_t)(n * a.h + iy) * a.w) * a.c + c;
            float win[7];
            win[0] = 0.f;
#pragma unroll
            for (int k = 1; k < 7; ++k) {      // the window of pixel x0 - 1, so that the first shift lands on x0
                const int ix = x0 - 4 + k;
                win[k] = (ix >= 0 && ix < a.w) ? xr[(int64_t)ix * a.c] : 0.f;
            }
            for (int px = x0; px < x1; ++px) {
#pragma unroll
                for (int k = 0; k < 6; ++k) win[k] = win[k + 1];
                win[6] = px + 3 < a.w ? xr[(int64_t)(px + 3) * a.c] : 0.f;
                const float d = dr[(int64_t)px * a.c];
#pragma unroll
                for (int kx = 0; kx < 7; ++kx) acc[ky * 7 + kx] = fmaf(d, win[kx], acc[ky * 7 + kx]);
                if (ky == 3) acc[49] += d;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 50; ++t) a.partial[((int64_t)strip * 50 + t) * a.c + c] = acc[t];
}

// grid (ceil(units / 4), ceil(C / 64)): one wave per (row, segment) unit
__global__ void __launch_bounds__(kCbThreads) cnb_dw_dgrad_kernel(CbDw a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int u = blockIdx.x * 4 + wave, c = blockIdx.y * 64 + lane;
    if (u >= a.units || c >= a.c) return;
    const int seg = u % a.nseg, rowi = u / a.nseg, y = rowi % a.h, n = rowi / a.h;
    const int x0 = seg * kCbSeg, x1 = min(a.w, x0 + kCbSeg);
    float wt[49], win[49];
#pragma unroll
    for (int j = 0; j < 49; ++j) wt[j] = a.taps[(int64_t)(48 - j) * a.c + c];   // the transposed taps
    const float *img = a.dz + ((int64_t)n * a.h * a.w) * a.c + c;
#pragma unroll
    for (int jy = 0; jy < 7; ++jy) {
        const int iy = y + jy - 3;
        const bool in = iy >= 0 && iy < a.h;
        win[jy * 7] = 0.f;
#pragma unroll
        for (int k = 1; k < 7; ++k) {
            const int ix = x0 - 4 + k;
            win[jy * 7 + k] = (in && ix >= 0 && ix < a.w) ? img[((int64_t)iy * a.w + ix) * a.c] : 0.f;
        }
    }
    for (int px = x0; px < x1; ++px) {
        float v = 0.f;
#pragma unroll
        for (int jy = 0; jy < 7; ++jy) {
            const int iy = y + jy - 3;
#pragma unroll
            for (int k = 0; k < 6; ++k) win[jy * 7 + k] = win[jy * 7 + k + 1];
            win[jy * 7 + 6] = (iy >= 0 && iy < a.h && px + 3 < a.w) ? img[((int64_t)iy * a.w + px + 3) * a.c] : 0.f;
#pragma unroll
            for (int jx = 0; jx < 7; ++jx) v = fmaf(win[jy * 7 + jx], wt[jy * 7 + jx], v);
        }
        const int64_t e = ((int64_t)(n * a.h + y) * a.w + px) * a.c + c;
        if (a.add) v += a.add[e];
        a.out[e] = v;
    }
}

// one workgroup per output channel c of the folded Linear: see kind 7
__global__ void __launch_bounds__(256) cnb_scale_kernel(const float *dwp, const float *w, const float *b, const float *g,
                                                        const float *dbp, int k, float *dw, float *db, float *dg)
{
    __shared__ float red[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    const float gc = g[c];
    float s = 0.f;
    for (int i = tid; i < k; i += 256) {
        const float t = dwp[(int64_t)c * k + i];
        s = fmaf(t, w[(int64_t)c * k + i], s);
        if (dw) dw[(int64_t)c * k + i] = gc * t;
    }
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        if (db) db[c] = gc * dbp[c];
        if (dg) dg[c] = fmaf(dbp[c], b[c], red[0]);
    }
}

// x [B, H, W, C] -> out [B, H / 2, W / 2, 4 C]; one thread per output quad
template <bool X3>
__global__ void __launch_bounds__(256) cnb_patches_kernel(const char *x, char *out, int batch, int h, int w, int c)
{
    const int nq = c >> 2, ho = h / 2, wo = w / 2;
    const int64_t total = (int64_t)batch * ho * wo * 4 * nq, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int q = (int)(i % nq);
        int64_t r = i / nq;
        const int tap = (int)(r & 3);
        r >>= 2;
        const int ox = (int)(r % wo), oy = (int)((r / wo) % ho), n = (int)(r / ((int64_t)wo * ho));
        const int64_t src = (((int64_t)n * h + 2 * oy + (tap >> 1)) * w + 2 * ox + (tap & 1)) * c + 4 * q;
        if (X3) *reinterpret_cast<float4 *>(out + i * 16) = *reinterpret_cast<const float4 *>(x + src * 4);
        else *reinterpret_cast<uint2 *>(out + i * 8) = *reinterpret_cast<const uint2 *>(x + src * 2);
    }
}

// dz [B, H / 2, W / 2, 4 C] -> out [B, H, W, C], zeros on the cropped pixels; one thread per output quad
template <bool X3>
__global__ void __launch_bounds__(256) cnb_pixels_kernel(const char *dz, char *out, int batch, int h, int w, int c)
{
    const int nq = c >> 2, ho = h / 2, wo = w / 2;
    const int64_t total = (int64_t)batch * h * w * nq, stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
        const int q = (int)(i % nq);
        const int64_t r = i / nq;
        const int px = (int)(r % w), py = (int)((r / w) % h), n = (int)(r / ((int64_t)w * h));
        const bool in = py < 2 * ho && px < 2 * wo;
        const int64_t src = ((((int64_t)n * ho + py / 2) * wo + px / 2) * 4 + (py & 1) * 2 + (px & 1)) * c + 4 * q;
        if (X3) *reinterpret_cast<float4 *>(out + i * 16) =
                    in ? *reinterpret_cast<const float4 *>(dz + src * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        else *reinterpret_cast<uint2 *>(out + i * 8) = in ? *reinterpret_cast<const uint2 *>(dz + src * 2) : make_uint2(0u, 0u);
    }
}

// g f32 [B, C, HW] -> out f32 [B, HW, C] = g (+ add); 32 pixels x 32 channels per block
__global__ void __launch_bounds__(256) cnb_ingest_kernel(const float *g, const float *add, int C, int HW, float *out)
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
        if (add) v += add[e];
        out[e] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------ host
const char *kind_name(int kind)
{
    static const char *names[] = {"dgrad", "wgrad", "rows", "gelu", "layer norm", "depthwise wgrad", "depthwise dgrad",
                                  "layer scale", "patches", "pixels", "ingest"};
    return kind >= 0 && kind <= 10 ? names[kind] : "?";
}

sdetr_backbone_bwd_op gemm_op(const sdetr_convnext_bwd_op &o)
{
    sdetr_backbone_bwd_op b = {};
    b.kind = o.kind;
    b.dz = o.dz;
    b.x = o.x;
    b.weight = o.weight;
    b.scale = o.scale;
    b.out = o.out;
    b.batch = o.batch;
    b.in_channels = o.channels;
    b.height = o.height;
    b.width = o.width;
    b.out_channels = o.out_channels;
    b.kernel_size = 1;
    b.stride = 1;
    b.padding = 0;
    b.splits = o.splits;
    return b;
}

struct CbPlan {
    int strips, chunks;
    int64_t rows, need;
};

int strips_for(int requested, int64_t most, int automatic)
{
    const int64_t want = requested > 0 ? requested : automatic;
    return (int)std::max<int64_t>(1, std::min<int64_t>(want, most));
}

// validation of one op without a launch
int check_op(const sdetr_convnext_bwd_op &o, int precision, CbPlan &p)
{
    p = CbPlan{};
    const char *name = kind_name(o.kind);
    if (o.kind < 0 || o.kind > 10) return fail("sdetr_convnext_bwd: unknown op kind %d", o.kind);
    if (precision != 0 && precision != 1) return fail("sdetr_convnext_bwd (%s): precision must be 0 or 1", name);
    if (o.kind <= 1) {
        if (o.add || o.gamma || o.dbias || o.dgamma || o.dbeta)
            return fail("sdetr_convnext_bwd (%s): a GEMM kind takes dz, x / weight, scale and out only", name);
        if (!all_aligned16(o.dz, o.x, o.weight, o.scale, o.out))
            return fail("sdetr_convnext_bwd (%s): tensors must be 16-byte aligned", name);
        const sdetr_backbone_bwd_op b = gemm_op(o);
        p.need = sdetr_backbone_bwd_workspace_bytes(&b, 1, precision);
        return p.need < 0 ? SDETR_EINVAL : 0;
    }
    if (o.batch < 1 || o.height < 1 || o.width < 1 || o.channels < 1 || o.splits < 0)
        return fail("sdetr_convnext_bwd (%s): bad shape (batch %d, %d x %d, channels %d, splits %d)", name, o.batch, o.height,
                    o.width, o.channels, o.splits);
    if (o.channels % 32) return fail("sdetr_convnext_bwd (%s): channels must be a multiple of 32 (got %d)", name, o.channels);
    if (o.kind >= 4 && o.kind <= 6 && o.channels > kCbMaxC)
        return fail("sdetr_convnext_bwd (%s): channels must be a multiple of 32 up to %d (got %d)", name, kCbMaxC, o.channels);
    p.rows = (int64_t)o.batch * o.height * o.width;
    if (p.rows * o.channels >= (int64_t(1) << 31) || p.rows >= (int64_t(1) << 30))
        return fail("sdetr_convnext_bwd (%s): tensors too large", name);
    if (!all_aligned16(o.dz, o.x, o.weight, o.scale, o.gamma, o.add, o.out, o.dbias, o.dgamma, o.dbeta))
        return fail("sdetr_convnext_bwd (%s): tensors must be 16-byte aligned", name);
    bool null = !o.out && o.kind != 7;
    const int c = o.channels;
    switch (o.kind) {
    case 2:
        null |= !o.dz;
        p.chunks = (c / 4 + 63) / 64;
        p.strips = strips_for(o.splits, (p.rows + 3) / 4, std::max(1, 1024 / p.chunks));
        p.need = (int64_t)p.strips * c * 4;
        break;
    case 3:
        null |= !o.dz || !o.x;
        p.chunks = (c / 4 + 63) / 64;
        p.strips = strips_for(o.splits, (p.rows + 3) / 4, std::max(1, 1024 / p.chunks));
        p.need = (int64_t)p.strips * c * 4;
        break;
    case 4:
        null |= !o.dz || !o.x || !o.gamma || (!o.dgamma != !o.dbeta);
        p.strips = strips_for(o.splits, (p.rows + 3) / 4, 512);
        p.need = (int64_t)p.strips * 2 * c * 4;
        break;
    case 5: {
        null |= !o.dz || !o.x;
        p.chunks = (c + 63) / 64;
        const int64_t units = (int64_t)o.batch * o.height * ((o.width + kCbSeg - 1) / kCbSeg);
        int automatic = std::max(4, 2048 / p.chunks);
        automatic -= automatic % 4;               // whole workgroups of four waves
        p.strips = strips_for(o.splits, units, automatic);
        p.need = (int64_t)p.strips * 50 * c * 4;
        break;
    }
    case 6:
        null |= !o.dz || !o.weight;
        p.chunks = (c + 63) / 64;
        break;
    case 7:
        null |= !o.dz || !o.x || !o.weight || !o.scale || !o.gamma;
        if (o.out_channels < 1) return fail("sdetr_convnext_bwd (%s): bad out_channels %d", name, o.out_channels);
        break;
    case 8:
        null |= !o.x;
        if (o.height < 2 || o.width < 2) return fail("sdetr_convnext_bwd (%s): no 2x2 patch in %d x %d", name, o.height, o.width);
        break;
    case 9:
        null |= !o.dz;
        if (o.height < 2 || o.width < 2) return fail("sdetr_convnext_bwd (%s): no 2x2 patch in %d x %d", name, o.height, o.width);
        break;
    default:
        null |= !o.dz;
        if (o.batch > 65535 || c / 32 > 65535) return fail("sdetr_convnext_bwd (%s): batch / channels too large", name);
        break;
    }
    if (null) return fail("sdetr_convnext_bwd (%s): null tensor", name);
    return 0;
}

int check_bwd_op(const sdetr_convnext_bwd_op &o, int precision, int64_t &need)
{
    CbPlan p;
    const int rc = check_op(o, precision, p);
    need = rc ? 0 : p.need;
    return rc;
}

template <bool X3>
void launch_kind(hipStream_t s, const sdetr_convnext_bwd_op &o, const CbPlan &p, void *ws)
{
    const int c = o.channels;
    float *partial = reinterpret_cast<float *>(ws);
    const char *dz = reinterpret_cast<const char *>(o.dz), *x = reinterpret_cast<const char *>(o.x);
    char *out = reinterpret_cast<char *>(o.out);
    if (o.kind == 2 || o.kind == 3) {
        const CbRows a = {dz, x, o.scale, out, partial, p.rows, c, o.height * o.width};
        const dim3 grid((unsigned)p.strips, (unsigned)p.chunks);
        if (o.kind == 2) hipLaunchKernelGGL((cnb_rows_kernel<X3, 2>), grid, dim3(kCbThreads), 0, s, a);
        else hipLaunchKernelGGL((cnb_rows_kernel<X3, 3>), grid, dim3(kCbThreads), 0, s, a);
        if (o.dbias)
            hipLaunchKernelGGL(cnb_sum_kernel, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, s, partial, p.strips, c, c, o.dbias,
                               (float *)nullptr);
    } else if (o.kind == 4) {
        static DeviceOnce once;
        allow_dynamic_lds(cnb_ln_kernel<X3>, once, 32 * kCbMaxC);
        const CbLn a = {dz, reinterpret_cast<const float *>(o.x), o.gamma, o.add, reinterpret_cast<float *>(o.out), partial, p.rows,
                        c, o.eps};
        hipLaunchKernelGGL(cnb_ln_kernel<X3>, dim3((unsigned)p.strips), dim3(kCbThreads), 32 * c, s, a);
        if (o.dgamma)
            hipLaunchKernelGGL(cnb_sum_kernel, dim3((unsigned)((2 * c + 255) / 256)), dim3(256), 0, s, partial, p.strips, 2 * c, c,
                               o.dgamma, o.dbeta);
    } else if (o.kind == 8) {
        const int64_t total = (int64_t)o.batch * (o.height / 2) * (o.width / 2) * c;
        const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 8192);
        hipLaunchKernelGGL(cnb_patches_kernel<X3>, dim3(blocks), dim3(256), 0, s, x, out, o.batch, o.height, o.width, c);
    } else {
        const int64_t total = p.rows * (c / 4);
        const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 8192);
        hipLaunchKernelGGL(cnb_pixels_kernel<X3>, dim3(blocks), dim3(256), 0, s, dz, out, o.batch, o.height, o.width, c);
    }
}

int run_bwd_op(hipStream_t s, const sdetr_convnext_bwd_op &o, int precision, void *ws, int64_t ws_bytes)
{
    CbPlan p;
    if (int rc = check_op(o, precision, p)) return rc;
    const char *name = kind_name(o.kind);
    if (p.need > ws_bytes || (p.need && !ws))
        return fail("sdetr_convnext_bwd (%s): workspace of %lld bytes is too small (%lld needed)", name, (long long)ws_bytes,
                    (long long)p.need);
    const int c = o.channels;
    if (o.kind <= 1) {
        const sdetr_backbone_bwd_op b = gemm_op(o);
        return o.kind == 0 ? sdetr_backbone_dgrad((sdetr_stream_t)s, &b, precision, ws, ws_bytes)
                           : sdetr_backbone_wgrad((sdetr_stream_t)s, &b, precision, ws, ws_bytes);
    }
    if (o.kind == 5 || o.kind == 6) {
        CbDw a = {};
        a.dz = reinterpret_cast<const float *>(o.dz);
        a.x = reinterpret_cast<const float *>(o.x);
        a.taps = reinterpret_cast<const float *>(o.weight);
        a.add = o.add;
        a.out = reinterpret_cast<float *>(o.out);
        a.partial = reinterpret_cast<float *>(ws);
        a.batch = o.batch;
        a.h = o.height;
        a.w = o.width;
        a.c = c;
        a.nseg = (o.width + kCbSeg - 1) / kCbSeg;
        a.units = o.batch * o.height * a.nseg;
        a.strips = p.strips;
        if (o.kind == 5) {
            hipLaunchKernelGGL(cnb_dw_wgrad_kernel, dim3((unsigned)((p.strips + 3) / 4), (unsigned)p.chunks), dim3(kCbThreads), 0,
                               s, a);
            hipLaunchKernelGGL(cnb_sum_kernel, dim3((unsigned)((50 * c + 255) / 256)), dim3(256), 0, s, a.partial, p.strips,
                               50 * c, 49 * c, a.out, o.dbias);
        } else {
            hipLaunchKernelGGL(cnb_dw_dgrad_kernel, dim3((unsigned)((a.units + 3) / 4), (unsigned)p.chunks), dim3(kCbThreads), 0, s,
                               a);
        }
    } else if (o.kind == 7) {
        hipLaunchKernelGGL(cnb_scale_kernel, dim3((unsigned)c), dim3(256), 0, s, reinterpret_cast<const float *>(o.x),
                           reinterpret_cast<const float *>(o.weight), o.scale, o.gamma, reinterpret_cast<const float *>(o.dz),
                           o.out_channels, reinterpret_cast<float *>(o.out), o.dbias, o.dgamma);
    } else if (o.kind == 10) {
        const int HW = o.height * o.width;
        hipLaunchKernelGGL(cnb_ingest_kernel, dim3((unsigned)((HW + 31) / 32), (unsigned)(c / 32), (unsigned)o.batch), dim3(256), 0,
                           s, reinterpret_cast<const float *>(o.dz), o.add, c, HW, reinterpret_cast<float *>(o.out));
    } else if (precision == 0) {
        launch_kind<true>(s, o, p, ws);
    } else {
        launch_kind<false>(s, o, p, ws);
    }
    return check_launch("sdetr_convnext_bwd");
}

}  // namespace
}  // namespace sdetr

using namespace sdetr;

using ConvnextBwdPlan = Plan<sdetr_convnext_bwd_op, check_bwd_op, run_bwd_op>;

extern "C" int64_t sdetr_convnext_bwd_workspace_bytes(const sdetr_convnext_bwd_op *ops, int n_ops, int precision)
{
    return ConvnextBwdPlan::workspace_bytes(ops, n_ops, precision);
}

extern "C" int sdetr_convnext_bwd_op_run(sdetr_stream_t stream, const sdetr_convnext_bwd_op *op, int precision,
                                         void *workspace, int64_t workspace_bytes)
{
    return ConvnextBwdPlan::op_run("sdetr_convnext_bwd", stream, op, precision, workspace, workspace_bytes);
}

extern "C" int sdetr_convnext_bwd_run(sdetr_stream_t stream, const sdetr_convnext_bwd_op *ops, int n_ops, int precision,
                                      void *workspace, int64_t workspace_bytes)
{
    return ConvnextBwdPlan::run("sdetr_convnext_bwd", stream, ops, n_ops, precision, workspace, workspace_bytes);
}

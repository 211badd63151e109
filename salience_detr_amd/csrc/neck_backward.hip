// Training the RepVGGPluX neck (include/salience_hip.h section (13b)): the training-mode forward's BatchNorm and gate
// launches and the backward plan, all on fp32 token-major rows [batch, height * width, channels].  neck.hip holds the
// convolution kernel the forward (and the stride-1 3x3 backward-data) runs.
//   nt_stats_*      batch statistics: (count, mean, M2) per 64-row tile, merged in tile order; running statistics
//   nt_apply        normalise + affine (+ the second norm of a RepVGG block) (+ SiLU)
//   nt_gate_*       the attention-pooled gate, keeping logits, softmax normaliser, context, hidden vector and gate
//   nb_dgrad        grouped k x k backward-data, stride 1 | 2, a gather over flipped weights (plain FMA)
//   nb_wgrad_*      grouped k x k backward-weight: a 16 x 16 tile of (input, output) channels per workgroup and pixel
//                   chunk, every tap in registers (plain FMA), then the chunks in order into the parameter's layout
//   nb_norm_*       BatchNorm backward with the SiLU derivative in front, one or two norms on one incoming gradient
//   nb_gate_*       gate backward: per-image reductions in tile order, the C / 16 MLP inside the kernel
//   nb_upsample     nearest up-sampling backward, a gather with the forward's index rule
// No atomics: every sum has a fixed order.  Every launch writes every element of its outputs.  The column sums over pixels
// (statistics, norm and gate backward, the merge of the backward-weight chunks) accumulate in double and round once: a
// serial fp32 sum over 16700 pixels would carry its error, coherently, into every element below it.
#include "backbone_rows_core.h"

namespace sdetr {
namespace {

constexpr int kNtRows = 64;        // rows per tile of the column reductions
constexpr int kNtGatePix = 128;    // pixels per tile of the gate's reductions
constexpr int kNtHidden = 64;      // most hidden units of the gate's MLP
constexpr int64_t kNtWgradBudget = int64_t(32) << 20;   // bytes of backward-weight partials at most

inline int64_t nt_align(int64_t v) { return (v + 255) / 256 * 256; }
inline unsigned nt_grid(int64_t n)
{
    const int64_t blocks = (n + kBlock - 1) / kBlock;
    return (unsigned)(blocks < 1 ? 1 : (blocks > 16384 ? 16384 : blocks));
}
__host__ __device__ inline int saved_stride(int C) { return 2 * C + kNtHidden + 4; }

__device__ __forceinline__ float nt_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }

// ------------------------------------------------------------------------------------------------ statistics
// grid (tiles, ceil(C / 256)): thread = channel; part [tiles][3][C] = count, mean, M2 of the tile
__global__ void __launch_bounds__(kBlock) nt_stats_partial_kernel(const float *z, int ld, int64_t rows, int C, float *part)
{
    const int c = blockIdx.y * kBlock + threadIdx.x;
    if (c >= C) return;
    const int64_t r0 = (int64_t)blockIdx.x * kNtRows, r1 = min(rows, r0 + kNtRows);
    double s = 0.0;
    for (int64_t r = r0; r < r1; ++r) s += (double)z[r * ld + c];
    const float n = (float)(r1 - r0), mean = (float)(s / (double)n);
    double m2 = 0.0;
    for (int64_t r = r0; r < r1; ++r) {
        const double d = (double)z[r * ld + c] - (double)mean;
        m2 += d * d;
    }
    float *p = part + (int64_t)blockIdx.x * 3 * C;
    p[c] = n;
    p[C + c] = mean;
    p[2 * C + c] = (float)m2;
}

// grid (ceil(C / 256)): the tiles in tile order
__global__ void __launch_bounds__(kBlock) nt_stats_finish_kernel(const float *part, int tiles, int C, float eps, float momentum,
                                                                 float *running_mean, float *running_var, float *stats)
{
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= C) return;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    for (int t = 0; t < tiles; ++t) {
        const float *p = part + (int64_t)t * 3 * C;
        const double nb = p[c], mb = p[C + c], m2b = p[2 * C + c];
        const double tot = n + nb, delta = mb - mean;
        mean += delta * (nb / tot);
        m2 += m2b + delta * delta * (n * nb / tot);
        n = tot;
    }
    stats[c] = (float)mean;
    stats[C + c] = (float)(1.0 / sqrt(m2 / n + (double)eps));
    if (running_mean) {
        running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * (float)mean;
        const float unbiased = (float)(n > 1.0 ? m2 / (n - 1.0) : m2 / n);
        running_var[c] = (1.0f - momentum) * running_var[c] + momentum * unbiased;
    }
}

struct ApplyArgs {
    const float *z, *stats, *gamma, *beta, *z2, *stats2, *gamma2, *beta2;
    float *out;
    int64_t rows;
    int C, ld_z, ld_out, act;
    float alpha;
};

__device__ __forceinline__ float nt_silu(float v) { return v * nt_sigmoid(v); }

__global__ void __launch_bounds__(kBlock) nt_apply_kernel(ApplyArgs a)
{
    const int64_t n = a.rows * a.C;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = e / a.C;
        const int c = (int)(e - row * a.C);
        float t = a.gamma[c] * ((a.z[row * a.ld_z + c] - a.stats[c]) * a.stats[a.C + c]) + a.beta[c];
        if (a.z2)
            t += a.alpha * (a.gamma2[c] * ((a.z2[row * a.ld_z + c] - a.stats2[c]) * a.stats2[a.C + c]) + a.beta2[c]);
        a.out[row * a.ld_out + c] = a.act ? nt_silu(t) : t;
    }
}

// ------------------------------------------------------------------------------------------------ gate, forward
// logit of pixel p (a wave per pixel, lane l channels l, l + 64, ..): every lane returns the sum
__device__ __forceinline__ float nt_row_dot(const float *row, const float *v, int C, int lane)
{
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s = fmaf(row[c], v[c], s);
    return wave_sum(s);
}

// grid (tiles, batch): part [batch][tiles][C + 2] = sum_p exp(l_p - max) y_p | max | sum_p exp(l_p - max)
__global__ void __launch_bounds__(kBlock) nt_gate_partial_kernel(const float *y, const float *mask, const float *mask_bias, int P,
                                                                int C, int tiles, float *logits, float *part)
{
    __shared__ float lg[kNtGatePix];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int p0 = t * kNtGatePix, n = min(kNtGatePix, P - p0);
    const float *yb = y + ((int64_t)b * P + p0) * C;
    const float bias = mask_bias ? mask_bias[0] : 0.f;
    for (int i = wave; i < n; i += kBlock / 64) {
        const float l = nt_row_dot(yb + (int64_t)i * C, mask, C, lane) + bias;
        if (lane == 0) {
            lg[i] = l;
            logits[(int64_t)b * P + p0 + i] = l;
        }
    }
    __syncthreads();
    float m = lg[0];
    for (int i = 1; i < n; ++i) m = fmaxf(m, lg[i]);
    float *dst = part + ((int64_t)b * tiles + t) * (C + 2);
    if (tid < C) {
        double v = 0.0;
        for (int i = 0; i < n; ++i) v += (double)expf(lg[i] - m) * (double)yb[(int64_t)i * C + tid];
        dst[tid] = (float)v;
    }
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += (double)expf(lg[i] - m);
        dst[C] = m;
        dst[C + 1] = (float)s;
    }
}

// grid (batch): the tiles in tile order, then the MLP; saved = gate [C] | context [C] | hidden [64] | max, sum, 0, 0
__global__ void __launch_bounds__(kBlock) nt_gate_finish_kernel(const float *part, int tiles, int C, int R, const float *w1,
                                                               const float *w2, float *saved)
{
    __shared__ float ctx[kBlock];
    __shared__ float hid[kNtHidden];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *pb = part + (int64_t)b * tiles * (C + 2);
    float *sv = saved + (int64_t)b * saved_stride(C);
    float m = pb[C];
    for (int t = 1; t < tiles; ++t) m = fmaxf(m, pb[(int64_t)t * (C + 2) + C]);
    double sd = 0.0, v = 0.0;
    for (int t = 0; t < tiles; ++t) {
        const float *p = pb + (int64_t)t * (C + 2);
        const double f = (double)expf(p[C] - m);
        sd += (double)p[C + 1] * f;
        if (tid < C) v += (double)p[tid] * f;
    }
    const float s = (float)sd;
    if (tid < C) {
        ctx[tid] = (float)(v / sd);
        sv[C + tid] = ctx[tid];
    }
    __syncthreads();
    if (tid < kNtHidden) {
        float u = 0.f;
        if (tid < R)
            for (int c = 0; c < C; ++c) u = fmaf(w1[(int64_t)tid * C + c], ctx[c], u);
        hid[tid] = fmaxf(u, 0.f);
        sv[2 * C + tid] = hid[tid];
    }
    if (tid == 0) {
        sv[2 * C + kNtHidden] = m;
        sv[2 * C + kNtHidden + 1] = s;
        sv[2 * C + kNtHidden + 2] = 0.f;
        sv[2 * C + kNtHidden + 3] = 0.f;
    }
    __syncthreads();
    if (tid < C) {
        float o = 0.f;
        for (int r = 0; r < R; ++r) o = fmaf(w2[(int64_t)tid * R + r], hid[r], o);
        sv[tid] = nt_sigmoid(o);
    }
}

__global__ void __launch_bounds__(kBlock) nt_gate_apply_kernel(const float *y, const float *saved, const float *sc, int ld_sc,
                                                              const float *sc2, int ld_sc2, int64_t rows, int P, int C, float *out)
{
    const int64_t n = rows * C;
    const int ss = 2 * C + kNtHidden + 4;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = e / C;
        const int c = (int)(e - row * C);
        const int64_t b = row / P;
        float v = fmaf(saved[b * ss + c], y[e], sc[row * ld_sc + c]);
        if (sc2) v += sc2[row * ld_sc2 + c];
        out[e] = v;
    }
}

// ------------------------------------------------------------------------------------------------ backward-data
struct ConvGeo {
    int B, H, W, Ho, Wo, G, CiG, CoG, K, S;
};

// a thread per (input pixel, 4 input channels); weight [G][K][K][CoG][CiG], taps flipped
__global__ void __launch_bounds__(kBlock) nb_dgrad_kernel(const float *dz, const float *w, ConvGeo g, float *out)
{
    const int Cin = g.G * g.CiG, Cout = g.G * g.CoG, c4n = Cin / 4, pad = (g.K - 1) / 2;
    const int64_t n = (int64_t)g.B * g.H * g.W * c4n;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(e % c4n) * 4;
        int64_t pix = e / c4n;
        const int ix = (int)(pix % g.W);
        pix /= g.W;
        const int iy = (int)(pix % g.H);
        const int64_t b = pix / g.H;
        const int grp = c / g.CiG, ci = c - grp * g.CiG;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int ky = 0; ky < g.K; ++ky) {
            const int ty = iy - pad + ky;
            if (ty < 0 || ty % g.S) continue;
            const int oy = ty / g.S;
            if (oy >= g.Ho) continue;
            for (int kx = 0; kx < g.K; ++kx) {
                const int tx = ix - pad + kx;
                if (tx < 0 || tx % g.S) continue;
                const int ox = tx / g.S;
                if (ox >= g.Wo) continue;
                const float *d = dz + ((b * g.Ho + oy) * g.Wo + ox) * Cout + grp * g.CoG;
                const float *wt = w + (((int64_t)grp * g.K * g.K + ky * g.K + kx) * g.CoG) * g.CiG + ci;
                for (int co = 0; co < g.CoG; ++co) {
                    const float dv = d[co];
                    const float4 wv = *reinterpret_cast<const float4 *>(wt + (int64_t)co * g.CiG);
                    acc.x = fmaf(dv, wv.x, acc.x);
                    acc.y = fmaf(dv, wv.y, acc.y);
                    acc.z = fmaf(dv, wv.z, acc.z);
                    acc.w = fmaf(dv, wv.w, acc.w);
                }
            }
        }
        *reinterpret_cast<float4 *>(out + e * 4) = acc;
    }
}

// ------------------------------------------------------------------------------------------------ backward-weight
// grid (chunks, G * ci tiles * co tiles): thread (ci = tid / 16, co = tid % 16) of a 16 x 16 tile, every tap in registers;
// part [chunks][G][K * K][CiG][CoG]
template <int K>
__global__ void __launch_bounds__(kBlock) nb_wgrad_partial_kernel(const float *dz, const float *x, int ld_x, ConvGeo g,
                                                                 int64_t chunk_pixels, float *part)
{
    constexpr int T = K * K, pad = (K - 1) / 2;
    const int ci_tiles = (g.CiG + 15) / 16, co_tiles = (g.CoG + 15) / 16;
    int tile = blockIdx.y;
    const int cot = tile % co_tiles;
    tile /= co_tiles;
    const int cit = tile % ci_tiles;
    const int grp = tile / ci_tiles;
    const int ci = cit * 16 + (threadIdx.x >> 4), co = cot * 16 + (threadIdx.x & 15);
    if (ci >= g.CiG || co >= g.CoG) return;              // (no barrier below)
    const int Cout = g.G * g.CoG;
    const int64_t total = (int64_t)g.B * g.Ho * g.Wo;
    const int64_t q0 = (int64_t)blockIdx.x * chunk_pixels, q1 = min(total, q0 + chunk_pixels);
    float acc[T];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = 0.f;
    for (int64_t q = q0; q < q1; ++q) {
        const int ox = (int)(q % g.Wo);
        const int64_t r = q / g.Wo;
        const int oy = (int)(r % g.Ho);
        const int64_t b = r / g.Ho;
        const float dv = dz[q * Cout + grp * g.CoG + co];
#pragma unroll
        for (int ky = 0; ky < K; ++ky) {
            const int iy = oy * g.S + ky - pad;
            if (iy < 0 || iy >= g.H) continue;
#pragma unroll
            for (int kx = 0; kx < K; ++kx) {
                const int ix = ox * g.S + kx - pad;
                if (ix < 0 || ix >= g.W) continue;
                acc[ky * K + kx] = fmaf(x[((b * g.H + iy) * g.W + ix) * ld_x + grp * g.CiG + ci], dv, acc[ky * K + kx]);
            }
        }
    }
    float *p = part + (int64_t)blockIdx.x * g.G * T * g.CiG * g.CoG;
#pragma unroll
    for (int t = 0; t < T; ++t) p[(((int64_t)grp * T + t) * g.CiG + ci) * g.CoG + co] = acc[t];
}

// the chunks in order -> dW [G * CoG][CiG][K][K]
__global__ void __launch_bounds__(kBlock) nb_wgrad_finish_kernel(const float *part, int chunks, int G, int T, int CiG, int CoG,
                                                                float *dw)
{
    const int64_t n = (int64_t)G * T * CiG * CoG;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        double s = 0.0;
        for (int k = 0; k < chunks; ++k) s += (double)part[(int64_t)k * n + e];
        const int co = (int)(e % CoG);
        int64_t r = e / CoG;
        const int ci = (int)(r % CiG);
        r /= CiG;
        const int t = (int)(r % T);
        const int grp = (int)(r / T);
        dw[(((int64_t)grp * CoG + co) * CiG + ci) * T + t] = (float)s;
    }
}

// ------------------------------------------------------------------------------------------------ sum
__global__ void __launch_bounds__(kBlock) nb_sum_kernel(const float *a, const float *b, const float *c, int64_t n4, float *out)
{
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n4; e += (int64_t)gridDim.x * blockDim.x) {
        float4 v = reinterpret_cast<const float4 *>(a)[e];
        const float4 w = reinterpret_cast<const float4 *>(b)[e];
        v.x += w.x, v.y += w.y, v.z += w.z, v.w += w.w;
        if (c) {
            const float4 u = reinterpret_cast<const float4 *>(c)[e];
            v.x += u.x, v.y += u.y, v.z += u.z, v.w += u.w;
        }
        reinterpret_cast<float4 *>(out)[e] = v;
    }
}

// ------------------------------------------------------------------------------------------------ BatchNorm backward
struct NormArgs {
    const float *dy, *z, *stats, *gamma, *beta, *z2, *stats2, *gamma2, *beta2;
    float *out, *out2, *dgamma, *dbeta, *dgamma2, *dbeta2;
    float *part;    // [tiles][3][C]
    float *sums;    // [3][C]
    int64_t rows;
    int C, ld_dy, ld_z, ld_out, act, tiles;
    float alpha;
};

// dt = dy * silu'(t) and the normalised values of one element
__device__ __forceinline__ float nb_dt(const NormArgs &a, int64_t row, int c, float &xh, float &xh2)
{
    xh = (a.z[row * a.ld_z + c] - a.stats[c]) * a.stats[a.C + c];
    xh2 = 0.f;
    float t = a.gamma[c] * xh + a.beta[c];
    if (a.z2) {
        xh2 = (a.z2[row * a.ld_z + c] - a.stats2[c]) * a.stats2[a.C + c];
        t += a.alpha * (a.gamma2[c] * xh2 + a.beta2[c]);
    }
    float dt = a.dy[row * a.ld_dy + c];
    if (a.act) {
        const float sg = nt_sigmoid(t);
        dt *= sg * (1.f + t * (1.f - sg));
    }
    return dt;
}

// grid (tiles, ceil(C / 256))
__global__ void __launch_bounds__(kBlock) nb_norm_partial_kernel(NormArgs a)
{
    const int c = blockIdx.y * kBlock + threadIdx.x;
    if (c >= a.C) return;
    const int64_t r0 = (int64_t)blockIdx.x * kNtRows, r1 = min(a.rows, r0 + kNtRows);
    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int64_t r = r0; r < r1; ++r) {
        float xh, xh2;
        const float dt = nb_dt(a, r, c, xh, xh2);
        s1 += (double)dt;
        s2 += (double)dt * (double)xh;
        s3 += (double)dt * (double)xh2;
    }
    float *p = a.part + (int64_t)blockIdx.x * 3 * a.C;
    p[c] = (float)s1;
    p[a.C + c] = (float)s2;
    p[2 * a.C + c] = (float)s3;
}

// grid (ceil(C / 256))
__global__ void __launch_bounds__(kBlock) nb_norm_finish_kernel(NormArgs a)
{
    const int c = blockIdx.x * kBlock + threadIdx.x;
    if (c >= a.C) return;
    double d1 = 0.0, d2 = 0.0, d3 = 0.0;
    for (int t = 0; t < a.tiles; ++t) {
        const float *p = a.part + (int64_t)t * 3 * a.C;
        d1 += (double)p[c];
        d2 += (double)p[a.C + c];
        d3 += (double)p[2 * a.C + c];
    }
    const float s1 = (float)d1, s2 = (float)d2, s3 = (float)d3;
    a.sums[c] = s1;
    a.sums[a.C + c] = s2;
    a.sums[2 * a.C + c] = s3;
    if (a.dgamma) {
        a.dbeta[c] = s1;
        a.dgamma[c] = s2;
    }
    if (a.dgamma2) {
        a.dbeta2[c] = a.alpha * s1;
        a.dgamma2[c] = a.alpha * s3;
    }
}

__global__ void __launch_bounds__(kBlock) nb_norm_apply_kernel(NormArgs a)
{
    const int64_t n = a.rows * a.C;
    const float inv = 1.0f / (float)a.rows;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = e / a.C;
        const int c = (int)(e - row * a.C);
        float xh, xh2;
        const float dt = nb_dt(a, row, c, xh, xh2);
        const float m1 = a.sums[c] * inv;
        a.out[row * a.ld_out + c] = a.gamma[c] * a.stats[a.C + c] * (dt - m1 - xh * (a.sums[a.C + c] * inv));
        if (a.z2)
            a.out2[row * a.ld_out + c] =
                a.alpha * a.gamma2[c] * a.stats2[a.C + c] * (dt - m1 - xh2 * (a.sums[2 * a.C + c] * inv));
    }
}

// ------------------------------------------------------------------------------------------------ gate, backward
struct GateArgs {
    const float *dz, *y, *logits, *saved, *mask, *w1, *w2;
    float *out, *dmask, *dbias, *dw1, *dw2;
    float *part1;   // [B][tiles][C]: sum_p dz y
    float *mid;     // [B][C + 4]: dctx | dctx . ctx
    float *pw1;     // [B][R][C]
    float *pw2;     // [B][C][R]
    float *part2;   // [B][tiles][C + 4]: sum_p dl_p y_p | sum_p dl_p
    int B, P, C, R, tiles;
};

// grid (tiles, batch)
__global__ void __launch_bounds__(kBlock) nb_gate_dg_kernel(GateArgs a)
{
    const int t = blockIdx.x, b = blockIdx.y, c = threadIdx.x;
    if (c >= a.C) return;
    const int p0 = t * kNtGatePix, n = min(kNtGatePix, a.P - p0);
    const int64_t base = ((int64_t)b * a.P + p0) * a.C + c;
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += (double)a.dz[base + (int64_t)i * a.C] * (double)a.y[base + (int64_t)i * a.C];
    a.part1[((int64_t)b * a.tiles + t) * a.C + c] = (float)s;
}

// grid (batch): gate gradient in tile order, back through the MLP; the image's share of the MLP's weight gradients
__global__ void __launch_bounds__(kBlock) nb_gate_mid_kernel(GateArgs a)
{
    __shared__ float d_o[kBlock];
    __shared__ float d_u[kNtHidden];
    __shared__ float d_c[kBlock];
    const int b = blockIdx.x, tid = threadIdx.x, C = a.C, R = a.R;
    const float *sv = a.saved + (int64_t)b * saved_stride(C);
    const float *gate = sv, *ctx = sv + C, *hid = sv + 2 * C;
    d_o[tid] = 0.f;
    if (tid < C) {
        double dg = 0.0;
        for (int t = 0; t < a.tiles; ++t) dg += (double)a.part1[((int64_t)b * a.tiles + t) * C + tid];
        d_o[tid] = (float)dg * gate[tid] * (1.f - gate[tid]);
    }
    __syncthreads();
    if (tid < kNtHidden) {
        float dh = 0.f;
        if (tid < R) {
            for (int c = 0; c < C; ++c) dh = fmaf(a.w2[(int64_t)c * R + tid], d_o[c], dh);
            if (!(hid[tid] > 0.f)) dh = 0.f;
        }
        d_u[tid] = dh;
    }
    __syncthreads();
    d_c[tid] = 0.f;
    if (tid < C) {
        float v = 0.f;
        for (int r = 0; r < R; ++r) v = fmaf(a.w1[(int64_t)r * C + tid], d_u[r], v);
        d_c[tid] = v;
        a.mid[(int64_t)b * (C + 4) + tid] = v;
        for (int r = 0; r < R; ++r) {
            a.pw1[((int64_t)b * R + r) * C + tid] = d_u[r] * ctx[tid];
            a.pw2[((int64_t)b * C + tid) * R + r] = d_o[tid] * hid[r];
        }
    }
    __syncthreads();
    if (tid == 0) {
        double dd = 0.0;
        for (int c = 0; c < C; ++c) dd += (double)d_c[c] * (double)ctx[c];
        a.mid[(int64_t)b * (C + 4) + C] = (float)dd;
    }
}

// grid (tiles, batch): the gradient at y; the tile's share of d conv_mask
__global__ void __launch_bounds__(kBlock) nb_gate_apply_kernel(GateArgs a)
{
    __shared__ float dl_s[kNtGatePix];
    __shared__ float a_s[kNtGatePix];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, C = a.C;
    const int p0 = t * kNtGatePix, n = min(kNtGatePix, a.P - p0);
    const float *sv = a.saved + (int64_t)b * saved_stride(C);
    const float *mid = a.mid + (int64_t)b * (C + 4);
    const float m = sv[2 * C + kNtHidden], s = sv[2 * C + kNtHidden + 1], dd = mid[C];
    const float *yb = a.y + ((int64_t)b * a.P + p0) * C;
    for (int i = wave; i < n; i += kBlock / 64) {
        const float e = nt_row_dot(yb + (int64_t)i * C, mid, C, lane);
        if (lane == 0) {
            const float ap = expf(a.logits[(int64_t)b * a.P + p0 + i] - m) / s;
            a_s[i] = ap;
            dl_s[i] = ap * (e - dd);
        }
    }
    __syncthreads();
    float *dst = a.part2 + ((int64_t)b * a.tiles + t) * (C + 4);
    if (tid < C) {
        const float g = sv[tid], dc = mid[tid], mk = a.mask[tid];
        const int64_t base = ((int64_t)b * a.P + p0) * C + tid;
        double acc = 0.0;
        for (int i = 0; i < n; ++i) {
            const int64_t e = base + (int64_t)i * C;
            a.out[e] = g * a.dz[e] + a_s[i] * dc + dl_s[i] * mk;
            acc += (double)dl_s[i] * (double)a.y[e];
        }
        dst[tid] = (float)acc;
    }
    if (tid == 0) {
        double acc = 0.0;
        for (int i = 0; i < n; ++i) acc += (double)dl_s[i];
        dst[C] = (float)acc;
    }
}

// grid (ceil(max(C, R * C) / 256)): images and tiles in order
__global__ void __launch_bounds__(kBlock) nb_gate_final_kernel(GateArgs a)
{
    const int e = blockIdx.x * kBlock + threadIdx.x, C = a.C, R = a.R;
    if (e < R * C) {
        float s1 = 0.f, s2 = 0.f;
        for (int b = 0; b < a.B; ++b) {
            s1 += a.pw1[(int64_t)b * R * C + e];
            s2 += a.pw2[(int64_t)b * R * C + e];
        }
        if (a.dw1) a.dw1[e] = s1;
        if (a.dw2) a.dw2[e] = s2;
    }
    if (e <= C && (e < C ? a.dmask != nullptr : a.dbias != nullptr)) {
        double s = 0.0;
        for (int b = 0; b < a.B; ++b)
            for (int t = 0; t < a.tiles; ++t) s += (double)a.part2[((int64_t)b * a.tiles + t) * (C + 4) + e];
        if (e < C) a.dmask[e] = (float)s;
        else a.dbias[0] = (float)s;
    }
}

// ------------------------------------------------------------------------------------------------ up-sampling backward
// a thread per (coarse pixel, 4 channels): the fine pixels whose nearest source it is, in row order
__global__ void __launch_bounds__(kBlock) nb_upsample_kernel(const float *dz, int B, int H, int W, int Hs, int Ws, int C, float *out)
{
    const int c4n = C / 4;
    const int64_t n = (int64_t)B * Hs * Ws * c4n;
    const float sh = (float)Hs / (float)H, sw = (float)Ws / (float)W;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(e % c4n) * 4;
        int64_t pix = e / c4n;
        const int xs = (int)(pix % Ws);
        pix /= Ws;
        const int ys = (int)(pix % Hs);
        const int64_t b = pix / Hs;
        const int y_lo = max(0, (int)((int64_t)ys * H / Hs) - 2), y_hi = min(H - 1, (int)(((int64_t)ys + 1) * H / Hs) + 2);
        const int x_lo = max(0, (int)((int64_t)xs * W / Ws) - 2), x_hi = min(W - 1, (int)(((int64_t)xs + 1) * W / Ws) + 2);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int yq = y_lo; yq <= y_hi; ++yq) {
            if (min((int)floorf((float)yq * sh), Hs - 1) != ys) continue;
            for (int xq = x_lo; xq <= x_hi; ++xq) {
                if (min((int)floorf((float)xq * sw), Ws - 1) != xs) continue;
                const float4 v = *reinterpret_cast<const float4 *>(dz + ((b * H + yq) * W + xq) * C + c);
                acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
            }
        }
        *reinterpret_cast<float4 *>(out + e * 4) = acc;
    }
}

// ------------------------------------------------------------------------------------------------------------ host
const char *kind_name(int kind)
{
    static const char *names[] = {"dgrad", "wgrad", "sum", "norm", "gate", "upsample"};
    return kind >= 0 && kind <= 5 ? names[kind] : "?";
}

int check_rows(const char *what, const sdetr_neck_bwd_op &o, int C)
{
    if (o.batch < 1 || o.height < 1 || o.width < 1 || C < 4 || (C % 4))
        return fail("%s: bad shape (batch %d, %d x %d, %d channels: a multiple of 4)", what, o.batch, o.height, o.width, C);
    if ((int64_t)o.batch * o.height * o.width * C >= (int64_t(1) << 40)) return fail("%s: map too large", what);
    return 0;
}

int check_conv(const char *what, const sdetr_neck_bwd_op &o, ConvGeo &g)
{
    if (int rc = check_rows(what, o, o.channels)) return rc;
    if ((o.kernel_size != 1 && o.kernel_size != 3) || (o.stride != 1 && o.stride != 2) || (o.kernel_size == 1 && o.stride != 1))
        return fail("%s: kernel %d / stride %d (3 with stride 1 | 2, or 1 with stride 1)", what, o.kernel_size, o.stride);
    if (o.groups < 1 || o.channels % o.groups || o.out_channels < 4 || o.out_channels % o.groups ||
        (o.channels / o.groups) % 4 || (o.out_channels / o.groups) % 4)
        return fail("%s: %d -> %d channels in %d groups (channels per group: multiples of 4)", what, o.channels, o.out_channels,
                    o.groups);
    g.B = o.batch, g.H = o.height, g.W = o.width, g.K = o.kernel_size, g.S = o.stride;
    g.Ho = (o.height - 1) / o.stride + 1, g.Wo = (o.width - 1) / o.stride + 1;
    g.G = o.groups, g.CiG = o.channels / o.groups, g.CoG = o.out_channels / o.groups;
    return 0;
}

struct NeckPlan {
    ConvGeo g;
    int chunks, tiles;
    int64_t chunk_pixels, off[5], need;
};

int wgrad_chunks(const sdetr_neck_bwd_op &o, const ConvGeo &g, NeckPlan &p)
{
    const int64_t pixels = (int64_t)g.B * g.Ho * g.Wo;
    const int64_t wsize = (int64_t)g.G * g.K * g.K * g.CiG * g.CoG * 4;
    int64_t chunks = o.splits > 0 ? o.splits : (pixels + 127) / 128;
    chunks = std::min<int64_t>(chunks, std::max<int64_t>(1, kNtWgradBudget / wsize));
    chunks = std::max<int64_t>(1, std::min<int64_t>(chunks, std::min<int64_t>(pixels, 1024)));
    p.chunk_pixels = (pixels + chunks - 1) / chunks;
    p.chunks = (int)((pixels + p.chunk_pixels - 1) / p.chunk_pixels);
    p.need = nt_align(wsize * p.chunks);
    return 0;
}

int check_op(const sdetr_neck_bwd_op &o, int precision, NeckPlan &p)
{
    p = NeckPlan{};
    if (o.kind < 0 || o.kind > 5) return fail("sdetr_neck_bwd: unknown op kind %d", o.kind);
    char what[64];
    snprintf(what, sizeof what, "sdetr_neck_bwd (%s)", kind_name(o.kind));
    if (precision != 0) return fail("%s: precision must be 0 (fp32 rows)", what);
    if (o.kind == 0) {
        if (int rc = check_conv(what, o, p.g)) return rc;
        if (!o.dz || !o.weight || !o.out) return fail("%s: null tensor", what);
        if (!all_aligned16(o.dz, o.weight, o.out)) return fail("%s: tensors must be 16-byte aligned", what);
        return 0;
    }
    if (o.kind == 1) {
        if (int rc = check_conv(what, o, p.g)) return rc;
        if (!o.dz || !o.x || !o.dweight) return fail("%s: null tensor", what);
        if (o.ld_x < o.channels) return fail("%s: ld_x %d < %d channels", what, o.ld_x, o.channels);
        return wgrad_chunks(o, p.g, p);
    }
    if (int rc = check_rows(what, o, o.channels)) return rc;
    const int64_t rows = (int64_t)o.batch * o.height * o.width;
    const int C = o.channels;
    if (o.kind == 2) {
        if (!o.dz || !o.add || !o.out) return fail("%s: null tensor", what);
        if (!all_aligned16(o.dz, o.add, o.x2, o.out)) return fail("%s: tensors must be 16-byte aligned", what);
        return 0;
    }
    if (o.kind == 3) {
        if (!o.dz || !o.x || !o.stats || !o.gamma || !o.beta || !o.out) return fail("%s: null tensor", what);
        if (o.x2 && (!o.stats2 || !o.gamma2 || !o.beta2 || !o.out2)) return fail("%s: null tensor of the second norm", what);
        if ((!o.dgamma != !o.dbeta) || (!o.dgamma2 != !o.dbeta2) || (!o.x2 && o.dgamma2))
            return fail("%s: dgamma and dbeta go together", what);
        if (o.ld_dz < C || o.ld_x < C || o.ld_out < C) return fail("%s: a row stride is below %d channels", what, C);
        if (o.act < 0 || o.act > 1) return fail("%s: bad act %d", what, o.act);
        p.tiles = (int)((rows + kNtRows - 1) / kNtRows);
        p.off[0] = nt_align((int64_t)p.tiles * 3 * C * 4);
        p.need = p.off[0] + nt_align((int64_t)3 * C * 4);
        return 0;
    }
    if (o.kind == 4) {
        if (C > kBlock || o.hidden < 1 || o.hidden > kNtHidden)
            return fail("%s: %d channels (at most 256), hidden width %d (1 .. 64)", what, C, o.hidden);
        if (!o.dz || !o.x || !o.x2 || !o.stats || !o.gamma || !o.weight || !o.weight2 || !o.out)
            return fail("%s: null tensor", what);
        if (o.batch > 65535) return fail("%s: batch too large", what);
        const int64_t P = (int64_t)o.height * o.width;
        if (P >= (int64_t(1) << 30)) return fail("%s: too many pixels", what);
        p.tiles = (int)((P + kNtGatePix - 1) / kNtGatePix);
        const int64_t B = o.batch;
        p.off[0] = nt_align(B * p.tiles * C * 4);
        p.off[1] = p.off[0] + nt_align(B * (C + 4) * 4);
        p.off[2] = p.off[1] + nt_align(B * o.hidden * C * 4);
        p.off[3] = p.off[2] + nt_align(B * o.hidden * C * 4);
        p.need = p.off[3] + nt_align(B * p.tiles * (C + 4) * 4);
        return 0;
    }
    if (o.src_height < 1 || o.src_width < 1 || o.src_height > o.height || o.src_width > o.width)
        return fail("%s: source %d x %d of a %d x %d map", what, o.src_height, o.src_width, o.height, o.width);
    if (!o.dz || !o.out) return fail("%s: null tensor", what);
    if (!all_aligned16(o.dz, o.out)) return fail("%s: tensors must be 16-byte aligned", what);
    return 0;
}

int check_bwd_op(const sdetr_neck_bwd_op &o, int precision, int64_t &need)
{
    NeckPlan p;
    const int rc = check_op(o, precision, p);
    need = rc ? 0 : p.need;
    return rc;
}

int run_bwd_op(hipStream_t s, const sdetr_neck_bwd_op &o, int precision, void *ws, int64_t ws_bytes)
{
    NeckPlan p;
    if (int rc = check_op(o, precision, p)) return rc;
    if (p.need > ws_bytes || (p.need && !ws))
        return fail("sdetr_neck_bwd (%s): workspace of %lld bytes is too small (%lld needed)", kind_name(o.kind),
                    (long long)ws_bytes, (long long)p.need);
    char *w = reinterpret_cast<char *>(ws);
    const int64_t rows = (int64_t)o.batch * o.height * o.width;
    const int C = o.channels;
    if (o.kind == 0) {
        const ConvGeo &g = p.g;
        if (g.K == 3 && g.S == 1)    // the forward kernel on the flipped, transposed weights
            return sdetr_neck_conv3x3((sdetr_stream_t)s, o.dz, SDETR_F32, g.B, g.H, g.W, g.G * g.CoG, o.weight, nullptr, g.G, g.CoG,
                                      g.CiG, 1, 0, o.out);
        hipLaunchKernelGGL(nb_dgrad_kernel, dim3(nt_grid(rows * (C / 4))), dim3(kBlock), 0, s, o.dz, o.weight, g, o.out);
    } else if (o.kind == 1) {
        const ConvGeo &g = p.g;
        const int tiles = g.G * ((g.CiG + 15) / 16) * ((g.CoG + 15) / 16);
        if (tiles > 65535) return fail("sdetr_neck_bwd (wgrad): too many channel tiles");
        float *part = reinterpret_cast<float *>(w);
        const dim3 grid((unsigned)p.chunks, (unsigned)tiles);
        if (g.K == 3)
            hipLaunchKernelGGL(nb_wgrad_partial_kernel<3>, grid, dim3(kBlock), 0, s, o.dz, o.x, o.ld_x, g, p.chunk_pixels, part);
        else
            hipLaunchKernelGGL(nb_wgrad_partial_kernel<1>, grid, dim3(kBlock), 0, s, o.dz, o.x, o.ld_x, g, p.chunk_pixels, part);
        const int T = g.K * g.K;
        hipLaunchKernelGGL(nb_wgrad_finish_kernel, dim3(nt_grid((int64_t)g.G * T * g.CiG * g.CoG)), dim3(kBlock), 0, s, part,
                           p.chunks, g.G, T, g.CiG, g.CoG, o.dweight);
    } else if (o.kind == 2) {
        hipLaunchKernelGGL(nb_sum_kernel, dim3(nt_grid(rows * C / 4)), dim3(kBlock), 0, s, o.dz, o.add, o.x2, rows * C / 4, o.out);
    } else if (o.kind == 3) {
        NormArgs a;
        a.dy = o.dz, a.z = o.x, a.stats = o.stats, a.gamma = o.gamma, a.beta = o.beta;
        a.z2 = o.x2, a.stats2 = o.stats2, a.gamma2 = o.gamma2, a.beta2 = o.beta2;
        a.out = o.out, a.out2 = o.out2, a.dgamma = o.dgamma, a.dbeta = o.dbeta, a.dgamma2 = o.dgamma2, a.dbeta2 = o.dbeta2;
        a.part = reinterpret_cast<float *>(w);
        a.sums = reinterpret_cast<float *>(w + p.off[0]);
        a.rows = rows, a.C = C, a.ld_dy = o.ld_dz, a.ld_z = o.ld_x, a.ld_out = o.ld_out, a.act = o.act, a.tiles = p.tiles;
        a.alpha = o.x2 ? o.alpha : 0.f;
        const unsigned cb = (unsigned)((C + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(nb_norm_partial_kernel, dim3((unsigned)p.tiles, cb), dim3(kBlock), 0, s, a);
        hipLaunchKernelGGL(nb_norm_finish_kernel, dim3(cb), dim3(kBlock), 0, s, a);
        hipLaunchKernelGGL(nb_norm_apply_kernel, dim3(nt_grid(rows * C)), dim3(kBlock), 0, s, a);
    } else if (o.kind == 4) {
        GateArgs a;
        a.dz = o.dz, a.y = o.x, a.logits = o.x2, a.saved = o.stats, a.mask = o.gamma, a.w1 = o.weight, a.w2 = o.weight2;
        a.out = o.out, a.dmask = o.dgamma, a.dbias = o.dbeta, a.dw1 = o.dweight, a.dw2 = o.dweight2;
        a.part1 = reinterpret_cast<float *>(w);
        a.mid = reinterpret_cast<float *>(w + p.off[0]);
        a.pw1 = reinterpret_cast<float *>(w + p.off[1]);
        a.pw2 = reinterpret_cast<float *>(w + p.off[2]);
        a.part2 = reinterpret_cast<float *>(w + p.off[3]);
        a.B = o.batch, a.P = o.height * o.width, a.C = C, a.R = o.hidden, a.tiles = p.tiles;
        const dim3 grid((unsigned)p.tiles, (unsigned)o.batch);
        hipLaunchKernelGGL(nb_gate_dg_kernel, grid, dim3(kBlock), 0, s, a);
        hipLaunchKernelGGL(nb_gate_mid_kernel, dim3((unsigned)o.batch), dim3(kBlock), 0, s, a);
        hipLaunchKernelGGL(nb_gate_apply_kernel, grid, dim3(kBlock), 0, s, a);
        const int most = std::max(C + 1, o.hidden * C);
        hipLaunchKernelGGL(nb_gate_final_kernel, dim3((unsigned)((most + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, a);
    } else {
        hipLaunchKernelGGL(nb_upsample_kernel, dim3(nt_grid((int64_t)o.batch * o.src_height * o.src_width * (C / 4))), dim3(kBlock),
                           0, s, o.dz, o.batch, o.height, o.width, o.src_height, o.src_width, C, o.out);
    }
    return check_launch("sdetr_neck_bwd");
}

}  // namespace
}  // namespace sdetr

using namespace sdetr;

using NeckBwdPlan = Plan<sdetr_neck_bwd_op, check_bwd_op, run_bwd_op>;

extern "C" int64_t sdetr_neck_bwd_workspace_bytes(const sdetr_neck_bwd_op *ops, int n_ops, int precision)
{
    return NeckBwdPlan::workspace_bytes(ops, n_ops, precision);
}

extern "C" int sdetr_neck_bwd_op_run(sdetr_stream_t stream, const sdetr_neck_bwd_op *op, int precision, void *workspace,
                                     int64_t workspace_bytes)
{
    return NeckBwdPlan::op_run("sdetr_neck_bwd", stream, op, precision, workspace, workspace_bytes);
}

extern "C" int sdetr_neck_bwd_run(sdetr_stream_t stream, const sdetr_neck_bwd_op *ops, int n_ops, int precision, void *workspace,
                                  int64_t workspace_bytes)
{
    return NeckBwdPlan::run("sdetr_neck_bwd", stream, ops, n_ops, precision, workspace, workspace_bytes);
}

extern "C" int64_t sdetr_neck_bn_stats_workspace_bytes(int64_t rows, int channels)
{
    if (rows < 1 || channels < 1) return 0;
    return nt_align(((rows + kNtRows - 1) / kNtRows) * 3 * channels * 4);
}

extern "C" int sdetr_neck_bn_stats(sdetr_stream_t stream, const float *z, int ld_z, int64_t rows, int channels, float eps,
                                   float momentum, float *running_mean, float *running_var, float *stats, void *workspace,
                                   int64_t workspace_bytes)
{
    if (rows < 1 || channels < 1 || ld_z < channels || rows >= (int64_t(1) << 36)) return fail("neck_bn_stats: bad sizes");
    if (!z || !stats || (!running_mean != !running_var)) return fail("neck_bn_stats: null pointer");
    if (!(eps >= 0.f)) return fail("neck_bn_stats: bad eps");
    const int64_t need = sdetr_neck_bn_stats_workspace_bytes(rows, channels);
    if (!workspace || workspace_bytes < need)
        return fail("neck_bn_stats: needs %lld bytes of workspace, got %lld", (long long)need, (long long)workspace_bytes);
    const int tiles = (int)((rows + kNtRows - 1) / kNtRows);
    const unsigned cb = (unsigned)((channels + kBlock - 1) / kBlock);
    float *part = reinterpret_cast<float *>(workspace);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(nt_stats_partial_kernel, dim3((unsigned)tiles, cb), dim3(kBlock), 0, s, z, ld_z, rows, channels, part);
    hipLaunchKernelGGL(nt_stats_finish_kernel, dim3(cb), dim3(kBlock), 0, s, part, tiles, channels, eps, momentum, running_mean,
                       running_var, stats);
    return check_launch("neck_bn_stats");
}

extern "C" int sdetr_neck_bn_apply(sdetr_stream_t stream, const float *z, const float *stats, const float *gamma,
                                   const float *beta, const float *z2, const float *stats2, const float *gamma2,
                                   const float *beta2, float alpha, int ld_z, int64_t rows, int channels, int activation,
                                   float *out, int ld_out)
{
    if (rows < 1 || channels < 1 || ld_z < channels || ld_out < channels) return fail("neck_bn_apply: bad sizes");
    if (!z || !stats || !gamma || !beta || !out) return fail("neck_bn_apply: null pointer");
    if (z2 && (!stats2 || !gamma2 || !beta2)) return fail("neck_bn_apply: null pointer of the second norm");
    if (activation < 0 || activation > 1) return fail("neck_bn_apply: bad activation %d", activation);
    ApplyArgs a;
    a.z = z, a.stats = stats, a.gamma = gamma, a.beta = beta, a.z2 = z2, a.stats2 = stats2, a.gamma2 = gamma2, a.beta2 = beta2;
    a.out = out, a.rows = rows, a.C = channels, a.ld_z = ld_z, a.ld_out = ld_out, a.act = activation, a.alpha = alpha;
    hipLaunchKernelGGL(nt_apply_kernel, dim3(nt_grid(rows * channels)), dim3(kBlock), 0, (hipStream_t)stream, a);
    return check_launch("neck_bn_apply");
}

extern "C" int64_t sdetr_neck_gate_train_workspace_bytes(int batch_size, int pixels, int channels)
{
    if (batch_size < 1 || pixels < 1 || channels < 1) return 0;
    const int64_t tiles = ((int64_t)pixels + kNtGatePix - 1) / kNtGatePix;
    return nt_align((int64_t)batch_size * tiles * (channels + 2) * 4);
}

extern "C" int sdetr_neck_gate_train(sdetr_stream_t stream, const float *y, int batch_size, int pixels, int channels,
                                     const float *mask_weight, const float *mask_bias, const float *squeeze_weight,
                                     const float *excite_weight, int hidden, const float *shortcut, int shortcut_row_stride,
                                     const float *shortcut2, int shortcut2_row_stride, float *logits, float *saved,
                                     void *workspace, int64_t workspace_bytes, float *out)
{
    if (batch_size < 1 || batch_size > 65535 || pixels < 1 || channels < 1 || channels > kBlock)
        return fail("neck_gate_train: bad sizes (at most 256 channels, got %d)", channels);
    if (hidden < 1 || hidden > kNtHidden) return fail("neck_gate_train: hidden width %d (1 .. 64)", hidden);
    if (shortcut_row_stride < channels || (shortcut2 && shortcut2_row_stride < channels))
        return fail("neck_gate_train: bad shortcut stride");
    if (!y || !mask_weight || !squeeze_weight || !excite_weight || !shortcut || !logits || !saved || !out)
        return fail("neck_gate_train: null pointer");
    const int64_t need = sdetr_neck_gate_train_workspace_bytes(batch_size, pixels, channels);
    if (!workspace || workspace_bytes < need)
        return fail("neck_gate_train: needs %lld bytes of workspace, got %lld", (long long)need, (long long)workspace_bytes);
    const int tiles = (pixels + kNtGatePix - 1) / kNtGatePix;
    float *part = reinterpret_cast<float *>(workspace);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(nt_gate_partial_kernel, dim3((unsigned)tiles, (unsigned)batch_size), dim3(kBlock), 0, s, y, mask_weight,
                       mask_bias, pixels, channels, tiles, logits, part);
    hipLaunchKernelGGL(nt_gate_finish_kernel, dim3((unsigned)batch_size), dim3(kBlock), 0, s, part, tiles, channels, hidden,
                       squeeze_weight, excite_weight, saved);
    const int64_t rows = (int64_t)batch_size * pixels;
    hipLaunchKernelGGL(nt_gate_apply_kernel, dim3(nt_grid(rows * channels)), dim3(kBlock), 0, s, y, saved, shortcut,
                       shortcut_row_stride, shortcut2, shortcut2_row_stride, rows, pixels, channels, out);
    return check_launch("neck_gate_train");
}

// Dense multi-head self-attention at ANY row count with an optional boolean mask, for the TRAINING step, forward and
// backward (fp32, 32-channel heads): the decoder layer's self-attention over its 900 matching queries plus the denoising
// queries (models/bricks/salience_transformer.py:566-573, nn.MultiheadAttention(256, 8) with q = k = query + pos,
// v = query, attn_mask = the denoising mask) between its in- and out-projection.
//
// The math and the decomposition are attention_train.hip's (that file serves the encoder's <= 512 unmasked rows with a
// head's whole K and V in LDS and stays as it is; its row helpers are restated here because the two files are separate
// translation units): 8 lanes per row, online softmax per lane, merged by three lane exchanges, the row's log-sum-exp
// saved, p = exp(s - lse) recomputed in the two backward kernels.  Two things are added.
//
// Tiles.  The forward and the dq kernel walk the KEYS in tiles of kAmTile = 128 rows of K and V staged in LDS; the dkv
//   kernel walks the QUERY rows in tiles of 128 rows of Q and dO (plus their lse and D = dO.o).  Each lane carries its own
//   (m, l, acc) -- or dq, or (dk, dv) -- across the tiles; the lanes of a row are merged once, after the last tile.
//   Why 128: a tile pair is 2 x 128 x 36 x 4 = 36,864 B (dkv: + 2 x 128 x 4 = 37,888 B), so the LDS never limits the
//   workgroups of a CU (four take 151,552 of its 160 KB); the registers do: 124 / 160 / 225 VGPRs (forward / dq / dkv, no
//   spill; forcing fewer spilled) admit 4 / 3 / 2 workgroups per CU.  At the training shape (2 images x 8 heads x ~1100 rows
//   = 560 workgroups of 32 rows) the forward and the dq kernel are then resident all at once on the 256 CUs (1024 / 768
//   places) and the dkv kernel nearly (512), instead of running in 2.2 rounds of one 147 KB workgroup per CU with T = 512;
//   and while one workgroup of a CU waits at its staging barrier the others compute, so the copy of the next tile needs no
//   double buffer.  A smaller tile only adds barriers.
//   Inside a tile lane `part` of a row takes the rows part, part + 8, ...: the 8 rows a 16-lane group of a 16-byte LDS read
//   touches are 36 floats apart, i.e. in 8 different 4-bank slots (36 p mod 64 = 0, 36, 8, 44, 16, 52, 24, 60).
// Mask.  `mask` [N, N] bytes (torch.bool storage as it lies), row = query, column = key, non-zero = NOT allowed, shared by
//   all images and heads; NULL = no mask.  A masked pair is SKIPPED: the mask byte decides, no arithmetic on -inf ever
//   does, and such a pair adds nothing to m, l, acc, dq, dk or dv.  A lane reads the (at most 16) mask bytes of its part of
//   a tile into one bit set before the tile's loop -- together with "this row exists" and "this key exists", so a row
//   past N in the last row block reads no mask byte at all.  A lane whose keys were all masked so far still has
//   m = -inf, l = 0, acc = 0; its first allowed key enters through `s > m` with exp(-inf - s) = 0, and exp(m - m) with both
//   infinite is never formed: the merge gives a lane with m = -inf the weight 0 without evaluating it.
//   A FULLY MASKED ROW (torch gives NaN; the reference's mask has none: its diagonal is always allowed) is defined here as:
//   output row 0, stored lse 0, and every gradient contribution of that row 0 (its pairs are all skipped in both backward
//   kernels).  Nothing is ever NaN or Inf for finite inputs.
//
//   forward      : workgroup = (32 query rows, head, image)
//   backward dq  : the same; dS = p (dO.v - D), D = dO.o
//   backward dkv : workgroup = (32 keys, head, image), 8 lanes per key over the query rows of a tile
// Every output element is written exactly once (no zero fill, no atomics, no workspace); no allocation and no host
// synchronisation in the entry points, so the three launches replay inside a captured graph.  Any N >= 0.
#include "common.h"

namespace sdetr {

constexpr int kAmD = 32, kAmRow = 36, kAmTile = 128, kAmThreads = 256;
constexpr int kAmLanes = 8;                                // lanes per row: each walks 1 / 8 of a tile
constexpr int kAmRowsPerBlock = kAmThreads / kAmLanes;    // 32
constexpr int kAmOwn = kAmD / kAmLanes;                    // channels a lane writes: 4
constexpr int kAmPer = kAmTile / kAmLanes;                 // tile rows per lane: 16 (one bit each in a lane's `allow` set)
static_assert(kAmPer <= 32 && kAmTile <= kAmThreads && 4 * (2 * kAmTile * kAmRow + 2 * kAmTile) * 4 <= 160 * 1024, "tile");

struct AmArgs {
    const float *q, *k, *v;       // element (b, n, h, c) at base + b * bs + n * rs + h * 32 + c
    int64_t q_bs, q_rs, k_bs, k_rs, v_bs, v_rs;
    const uint8_t *mask;          // [N, N] bytes, row stride mask_rs; non-zero = the pair is skipped; NULL = none
    int64_t mask_rs;
    float *o;                     // [B, N, H * 32]
    float *lse;                   // [B, H, N]
    const float *go;              // grad of o, [B, N, H * 32]
    float *gq, *gk, *gv;          // strides as q / k / v
    int B, H, N;
    float scale;
};

__device__ __forceinline__ void am_load_row(const float *src, float (&r)[kAmD])
{
#pragma unroll
    for (int i = 0; i < kAmD / 4; ++i) {
        const float4 v = reinterpret_cast<const float4 *>(src)[i];
        r[4 * i] = v.x; r[4 * i + 1] = v.y; r[4 * i + 2] = v.z; r[4 * i + 3] = v.w;
    }
}
__device__ __forceinline__ float am_dot(const float (&a)[kAmD], const float *lds_row)
{
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kAmD / 4; ++i) {
        const float4 v = reinterpret_cast<const float4 *>(lds_row)[i];
        s = fmaf(a[4 * i], v.x, s); s = fmaf(a[4 * i + 1], v.y, s); s = fmaf(a[4 * i + 2], v.z, s); s = fmaf(a[4 * i + 3], v.w, s);
    }
    return s;
}
__device__ __forceinline__ void am_axpy(float (&acc)[kAmD], float a, const float *lds_row)
{
#pragma unroll
    for (int i = 0; i < kAmD / 4; ++i) {
        const float4 v = reinterpret_cast<const float4 *>(lds_row)[i];
        acc[4 * i] = fmaf(a, v.x, acc[4 * i]); acc[4 * i + 1] = fmaf(a, v.y, acc[4 * i + 1]);
        acc[4 * i + 2] = fmaf(a, v.z, acc[4 * i + 2]); acc[4 * i + 3] = fmaf(a, v.w, acc[4 * i + 3]);
    }
}
// n <= kAmTile rows of a head's matrix (from `src`, row stride rs floats in global memory) into LDS rows of kAmRow floats:
// a full tile is 1024 float4, four in flight per thread
__device__ __forceinline__ void am_stage(const float *src, int64_t rs, int n, float *dst, int tid)
{
    const int total = n * (kAmD / 4);
    for (int t0 = tid; t0 < total; t0 += 4 * kAmThreads) {
        float4 r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = min(t0 + u * kAmThreads, total - 1);
            r[u] = reinterpret_cast<const float4 *>(src + (int64_t)(t >> 3) * rs)[t & 7];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int t = t0 + u * kAmThreads;
            if (t < total) reinterpret_cast<float4 *>(dst + (t >> 3) * kAmRow)[t & 7] = r[u];
        }
    }
}
// Bit t: the lane's t-th pair of this tile exists (t < count) and is allowed (its mask byte, at first + t * step, is 0;
// first == nullptr: no mask).  Only existing pairs are read.
__device__ __forceinline__ unsigned am_allowed(const uint8_t *first, int64_t step, int count)
{
    unsigned bits = 0;
#pragma unroll
    for (int t = 0; t < kAmPer; ++t)
        if (t < count && (first == nullptr || first[t * step] == 0)) bits |= 1u << t;
    return bits;
}
// how many of the tile's n rows lane `part` owns (rows part, part + 8, ... < n)
__device__ __forceinline__ int am_count(int n, int part) { return (n - part + kAmLanes - 1) >> 3; }
static_assert(kAmLanes == 8, "am_count shifts by log2(lanes)");

__global__ void __launch_bounds__(kAmThreads) attention_train_masked_fwd_kernel(AmArgs p)
{
    __shared__ __attribute__((aligned(16))) float ks[kAmTile * kAmRow];
    __shared__ __attribute__((aligned(16))) float vs[kAmTile * kAmRow];
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int part = tid & (kAmLanes - 1), i = blockIdx.x * kAmRowsPerBlock + tid / kAmLanes;
    const bool live = i < p.N;
    const int ii = live ? i : p.N - 1;
    float q[kAmD], acc[kAmD];
    am_load_row(p.q + (int64_t)b * p.q_bs + (int64_t)ii * p.q_rs + h * kAmD, q);
#pragma unroll
    for (int c = 0; c < kAmD; ++c) { q[c] *= p.scale; acc[c] = 0.f; }
    const uint8_t *mrow = p.mask ? p.mask + (int64_t)ii * p.mask_rs + part : nullptr;
    const float *kb = p.k + (int64_t)b * p.k_bs + h * kAmD, *vb = p.v + (int64_t)b * p.v_bs + h * kAmD;
    float m = -INFINITY, l = 0.f;
    for (int t0 = 0; t0 < p.N; t0 += kAmTile) {
        const int n = min(kAmTile, p.N - t0);
        if (t0) __syncthreads();   // the previous tile has been read
        am_stage(kb + (int64_t)t0 * p.k_rs, p.k_rs, n, ks, tid);
        am_stage(vb + (int64_t)t0 * p.v_rs, p.v_rs, n, vs, tid);
        const unsigned allow = am_allowed(mrow ? mrow + t0 : nullptr, kAmLanes, live ? am_count(n, part) : 0);
        __syncthreads();
        for (int t = 0; t < kAmPer; ++t) {
            if (!((allow >> t) & 1u)) continue;
            const int j = part + kAmLanes * t;
            const float s = am_dot(q, ks + j * kAmRow);
            if (s > m) {   // (rare after the first few keys; m = -inf before the lane's first allowed key: corr = 0)
                const float corr = expf(m - s);
                l *= corr;
#pragma unroll
                for (int c = 0; c < kAmD; ++c) acc[c] *= corr;
                m = s;
            }
            const float e = expf(s - m);
            l += e;
            am_axpy(acc, e, vs + j * kAmRow);
        }
    }
    // the parts of a row sit in adjacent lanes
    float m_all = m;
#pragma unroll
    for (int o = 1; o < kAmLanes; o <<= 1) m_all = fmaxf(m_all, __shfl_xor(m_all, o, kAmLanes));
    const float w = m == -INFINITY ? 0.f : expf(m - m_all);   // (a lane without an allowed key: nothing to add)
    l *= w;
#pragma unroll
    for (int o = 1; o < kAmLanes; o <<= 1) l += __shfl_xor(l, o, kAmLanes);
    const bool any = l > 0.f;                                  // false: a fully masked row -> output 0, lse 0
    const float inv = any ? 1.0f / l : 0.f;
    float mine[kAmOwn];
#pragma unroll
    for (int c = 0; c < kAmD; ++c) {
        float a = acc[c] * w;
#pragma unroll
        for (int o = 1; o < kAmLanes; o <<= 1) a += __shfl_xor(a, o, kAmLanes);
        if (c / kAmOwn == part) mine[c % kAmOwn] = a * inv;   // (c is a compile-time index: a select, not an indexed store)
    }
    if (live) {
        float *o = p.o + ((int64_t)b * p.N + i) * (p.H * kAmD) + h * kAmD + kAmOwn * part;
        reinterpret_cast<float4 *>(o)[0] = make_float4(mine[0], mine[1], mine[2], mine[3]);
        if (part == 0) p.lse[((int64_t)b * p.H + h) * p.N + i] = any ? m_all + logf(l) : 0.f;
    }
}

__global__ void __launch_bounds__(kAmThreads) attention_train_masked_bwd_dq_kernel(AmArgs p)
{
    __shared__ __attribute__((aligned(16))) float ks[kAmTile * kAmRow];
    __shared__ __attribute__((aligned(16))) float vs[kAmTile * kAmRow];
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int part = tid & (kAmLanes - 1), i = blockIdx.x * kAmRowsPerBlock + tid / kAmLanes;
    const bool live = i < p.N;
    const int ii = live ? i : p.N - 1;
    float q[kAmD], go[kAmD], dq[kAmD];
    am_load_row(p.q + (int64_t)b * p.q_bs + (int64_t)ii * p.q_rs + h * kAmD, q);
    const int64_t orow = ((int64_t)b * p.N + ii) * (p.H * kAmD) + h * kAmD;
    am_load_row(p.go + orow, go);
    float D = 0.f;
    {
        float o[kAmD];
        am_load_row(p.o + orow, o);
#pragma unroll
        for (int c = 0; c < kAmD; ++c) D = fmaf(go[c], o[c], D);
    }
    const float lse = p.lse[((int64_t)b * p.H + h) * p.N + ii];
#pragma unroll
    for (int c = 0; c < kAmD; ++c) { q[c] *= p.scale; dq[c] = 0.f; }
    const uint8_t *mrow = p.mask ? p.mask + (int64_t)ii * p.mask_rs + part : nullptr;
    const float *kb = p.k + (int64_t)b * p.k_bs + h * kAmD, *vb = p.v + (int64_t)b * p.v_bs + h * kAmD;
    for (int t0 = 0; t0 < p.N; t0 += kAmTile) {
        const int n = min(kAmTile, p.N - t0);
        if (t0) __syncthreads();
        am_stage(kb + (int64_t)t0 * p.k_rs, p.k_rs, n, ks, tid);
        am_stage(vb + (int64_t)t0 * p.v_rs, p.v_rs, n, vs, tid);
        const unsigned allow = am_allowed(mrow ? mrow + t0 : nullptr, kAmLanes, live ? am_count(n, part) : 0);
        __syncthreads();
        for (int t = 0; t < kAmPer; ++t) {
            if (!((allow >> t) & 1u)) continue;
            const int j = part + kAmLanes * t;
            const float pr = expf(am_dot(q, ks + j * kAmRow) - lse);
            const float ds = pr * (am_dot(go, vs + j * kAmRow) - D) * p.scale;
            am_axpy(dq, ds, ks + j * kAmRow);
        }
    }
    float mine[kAmOwn];
#pragma unroll
    for (int c = 0; c < kAmD; ++c) {
        float a = dq[c];
#pragma unroll
        for (int o = 1; o < kAmLanes; o <<= 1) a += __shfl_xor(a, o, kAmLanes);
        if (c / kAmOwn == part) mine[c % kAmOwn] = a;
    }
    if (live) {
        float *g = p.gq + (int64_t)b * p.q_bs + (int64_t)i * p.q_rs + h * kAmD + kAmOwn * part;
        reinterpret_cast<float4 *>(g)[0] = make_float4(mine[0], mine[1], mine[2], mine[3]);
    }
}

__global__ void __launch_bounds__(kAmThreads) attention_train_masked_bwd_dkv_kernel(AmArgs p)
{
    __shared__ __attribute__((aligned(16))) float qs[kAmTile * kAmRow];
    __shared__ __attribute__((aligned(16))) float gs[kAmTile * kAmRow];
    __shared__ float lse_s[kAmTile], d_s[kAmTile];
    const int tid = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int part = tid & (kAmLanes - 1), j = blockIdx.x * kAmRowsPerBlock + tid / kAmLanes;
    const bool live = j < p.N;
    const int jj = live ? j : p.N - 1;
    float k[kAmD], v[kAmD], dk[kAmD], dv[kAmD];
    am_load_row(p.k + (int64_t)b * p.k_bs + (int64_t)jj * p.k_rs + h * kAmD, k);
    am_load_row(p.v + (int64_t)b * p.v_bs + (int64_t)jj * p.v_rs + h * kAmD, v);
#pragma unroll
    for (int c = 0; c < kAmD; ++c) { k[c] *= p.scale; dk[c] = 0.f; dv[c] = 0.f; }
    // the key's COLUMN of the mask: the lane's query rows of a tile are 8 mask rows apart
    const uint8_t *mcol = p.mask ? p.mask + (int64_t)part * p.mask_rs + jj : nullptr;
    const float *qb = p.q + (int64_t)b * p.q_bs + h * kAmD;
    const int64_t hd = (int64_t)p.H * kAmD;
    const float *gb = p.go + (int64_t)b * p.N * hd + h * kAmD, *ob = p.o + (int64_t)b * p.N * hd + h * kAmD;
    const float *lb = p.lse + ((int64_t)b * p.H + h) * p.N;
    for (int t0 = 0; t0 < p.N; t0 += kAmTile) {
        const int n = min(kAmTile, p.N - t0);
        if (t0) __syncthreads();
        am_stage(qb + (int64_t)t0 * p.q_rs, p.q_rs, n, qs, tid);
        am_stage(gb + (int64_t)t0 * hd, hd, n, gs, tid);
        if (tid < n) {   // D = dO.o of the tile's rows, summed in am_dot's order: where o == v exactly (a row with one
                         // allowed key) dO.v - D is exactly 0, as it is in the dq kernel and in torch
            float go[kAmD], o[kAmD];
            am_load_row(gb + (int64_t)(t0 + tid) * hd, go);
            am_load_row(ob + (int64_t)(t0 + tid) * hd, o);
            float D = 0.f;
#pragma unroll
            for (int c = 0; c < kAmD; ++c) D = fmaf(go[c], o[c], D);
            d_s[tid] = D;
            lse_s[tid] = lb[t0 + tid];
        }
        const unsigned allow = am_allowed(mcol ? mcol + (int64_t)t0 * p.mask_rs : nullptr, kAmLanes * p.mask_rs,
                                          live ? am_count(n, part) : 0);
        __syncthreads();
        for (int t = 0; t < kAmPer; ++t) {
            if (!((allow >> t) & 1u)) continue;
            const int i = part + kAmLanes * t;
            const float pr = expf(am_dot(k, qs + i * kAmRow) - lse_s[i]);
            const float ds = pr * (am_dot(v, gs + i * kAmRow) - d_s[i]) * p.scale;
            am_axpy(dk, ds, qs + i * kAmRow);
            am_axpy(dv, pr, gs + i * kAmRow);
        }
    }
    float mk[kAmOwn], mv[kAmOwn];
#pragma unroll
    for (int c = 0; c < kAmD; ++c) {
        float a = dk[c], e = dv[c];
#pragma unroll
        for (int o = 1; o < kAmLanes; o <<= 1) { a += __shfl_xor(a, o, kAmLanes); e += __shfl_xor(e, o, kAmLanes); }
        if (c / kAmOwn == part) { mk[c % kAmOwn] = a; mv[c % kAmOwn] = e; }
    }
    if (live) {
        float *g = p.gk + (int64_t)b * p.k_bs + (int64_t)j * p.k_rs + h * kAmD + kAmOwn * part;
        reinterpret_cast<float4 *>(g)[0] = make_float4(mk[0], mk[1], mk[2], mk[3]);
        float *gv = p.gv + (int64_t)b * p.v_bs + (int64_t)j * p.v_rs + h * kAmD + kAmOwn * part;
        reinterpret_cast<float4 *>(gv)[0] = make_float4(mv[0], mv[1], mv[2], mv[3]);
    }
}

}  // namespace sdetr

using namespace sdetr;

static int am_check(int B, int H, int N, int head_dim, const AmArgs &a)
{
    if (head_dim != kAmD) return fail("attention_train_masked: built for 32-channel heads (got %d)", head_dim);
    if (B < 0 || H <= 0 || N < 0) return fail("attention_train_masked: bad sizes");
    if (B > 65535 || H > 65535) return fail("attention_train_masked: at most 65535 images and heads");
    const int64_t w = (int64_t)H * kAmD;
    if (a.q_rs < w || a.k_rs < w || a.v_rs < w || (a.q_rs & 3) || (a.k_rs & 3) || (a.v_rs & 3) || (a.q_bs & 3) || (a.k_bs & 3) ||
        (a.v_bs & 3))
        return fail("attention_train_masked: row strides must cover the heads and be multiples of 4 floats");
    if (a.mask && a.mask_rs < N) return fail("attention_train_masked: the mask's row stride (%lld) is below the %d rows",
                                             (long long)a.mask_rs, N);
    return 0;
}

extern "C" int sdetr_attention_train_masked_tile_rows(void) { return kAmTile; }

extern "C" int sdetr_attention_train_masked_forward_f32(sdetr_stream_t stream, const float *q, int64_t q_batch_stride,
                                                        int64_t q_row_stride, const float *k, int64_t k_batch_stride,
                                                        int64_t k_row_stride, const float *v, int64_t v_batch_stride,
                                                        int64_t v_row_stride, int batch_size, int num_heads, int num_rows,
                                                        int head_dim, float scale, const uint8_t *mask,
                                                        int64_t mask_row_stride, float *out, float *lse)
{
    AmArgs a{};
    a.q = q; a.k = k; a.v = v; a.q_bs = q_batch_stride; a.q_rs = q_row_stride; a.k_bs = k_batch_stride; a.k_rs = k_row_stride;
    a.v_bs = v_batch_stride; a.v_rs = v_row_stride; a.mask = mask; a.mask_rs = mask_row_stride; a.o = out; a.lse = lse;
    a.B = batch_size; a.H = num_heads; a.N = num_rows; a.scale = scale;
    if (int e = am_check(batch_size, num_heads, num_rows, head_dim, a)) return e;
    if ((int64_t)batch_size * num_rows == 0) return 0;
    if (!q || !k || !v || !out || !lse) return fail("attention_train_masked: null pointer");
    const dim3 grid((unsigned)((num_rows + kAmRowsPerBlock - 1) / kAmRowsPerBlock), (unsigned)num_heads, (unsigned)batch_size);
    hipLaunchKernelGGL(attention_train_masked_fwd_kernel, grid, dim3(kAmThreads), 0, static_cast<hipStream_t>(stream), a);
    return check_launch("attention_train_masked_forward");
}

extern "C" int sdetr_attention_train_masked_backward_f32(sdetr_stream_t stream, const float *q, int64_t q_batch_stride,
                                                         int64_t q_row_stride, const float *k, int64_t k_batch_stride,
                                                         int64_t k_row_stride, const float *v, int64_t v_batch_stride,
                                                         int64_t v_row_stride, int batch_size, int num_heads, int num_rows,
                                                         int head_dim, float scale, const uint8_t *mask,
                                                         int64_t mask_row_stride, const float *out, const float *lse,
                                                         const float *grad_out, float *grad_q, float *grad_k, float *grad_v)
{
    AmArgs a{};
    a.q = q; a.k = k; a.v = v; a.q_bs = q_batch_stride; a.q_rs = q_row_stride; a.k_bs = k_batch_stride; a.k_rs = k_row_stride;
    a.v_bs = v_batch_stride; a.v_rs = v_row_stride; a.mask = mask; a.mask_rs = mask_row_stride;
    a.o = const_cast<float *>(out); a.lse = const_cast<float *>(lse);
    a.go = grad_out; a.gq = grad_q; a.gk = grad_k; a.gv = grad_v; a.B = batch_size; a.H = num_heads; a.N = num_rows; a.scale = scale;
    if (int e = am_check(batch_size, num_heads, num_rows, head_dim, a)) return e;
    if ((int64_t)batch_size * num_rows == 0) return 0;
    if (!q || !k || !v || !out || !lse || !grad_out || !grad_q || !grad_k || !grad_v)
        return fail("attention_train_masked: null pointer");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((num_rows + kAmRowsPerBlock - 1) / kAmRowsPerBlock), (unsigned)num_heads, (unsigned)batch_size);
    hipLaunchKernelGGL(attention_train_masked_bwd_dq_kernel, grid, dim3(kAmThreads), 0, s, a);
    if (int e = check_launch("attention_train_masked_backward_dq")) return e;
    hipLaunchKernelGGL(attention_train_masked_bwd_dkv_kernel, grid, dim3(kAmThreads), 0, s, a);
    return check_launch("attention_train_masked_backward_dkv");
}

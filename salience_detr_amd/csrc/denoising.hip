// Contrastive denoising queries (reference models/bricks/denoising.py:GenerateCDNQueries) as ONE launch forward and ONE
// launch backward.
//
// Forward, cdn_queries_kernel.  The grid has two parts:
//  * row blocks: one wave per denoising slot (b, s), s = r * max_gt + t with repeat r in [0, 2 * groups) (even r: the
//    positive copy of group r / 2, odd r: the negative one) and target t of image b.  The wave reads the target from the
//    staged buffers of set_criterion.hip (boxes [B * capacity, 4] cxcywh, labels, offsets), its ten uniforms from
//    noise [2 * groups, B * capacity, 10] and writes
//      - the label row: label_encoder.weight[label'] copied as float4 per lane (bit-exact), label' = a random class when
//        u0 < label_noise_prob * 0.5 (apply_label_noise), floor(u1 * num_classes) clipped to num_classes - 1;
//      - the box (lane 0): cxcywh -> xyxy, += sign * (magnitude + [negative]) * (w/2, h/2, w/2, h/2) * box_noise_scale,
//        clamp to [0, 1], -> cxcywh, inverse sigmoid with eps = 1e-3 (apply_box_noise, util/misc.py:31-35), every
//        operation rounded on its own in the reference's order (no FMA contraction: torch runs them as separate kernels);
//      - noised_labels[b, s] = label' (saved for the backward).
//    Padding slots (t >= the image's count) get a zero label row, a zero box and label -1 from the kernel itself, so no
//    fill / memset has to run in front of the launch.  A slot whose staged row lies outside the staged buffers or whose
//    label lies outside [0, num_classes) is written as padding (nothing is read out of bounds).
//  * mask blocks: attn_mask [T, T] bytes, T = n_dn + num_queries, 1 = may not attend: allowed(i, j) iff j >= n_dn, or
//    i < n_dn and i, j lie in the same block of 2 * max_gt slots (generate_query_masks); 16 bytes per thread.
//
// Backward, cdn_label_grad_kernel: d weight[c] = sum of grad_label_queries[b, s] over the slots with noised_labels[b, s]
// == c.  One workgroup per class: wave 0 compacts the matching slots of the [B * n_dn] label table into an LDS list in
// table order (ballots), then thread = column adds the rows of the list in that order and writes the whole row of the
// class (zeros when the class never occurs).  No floating-point atomics, no memset, bit-identical from run to run.  The
// list is sized from the arguments (B * n_dn ints); a table too long for the LDS is walked in global memory by every
// thread instead (same order, same sums).
#include "common.h"

#pragma clang fp contract(off)

namespace sdetr {
namespace {

constexpr int kCdnRowsPerBlock = kBlock / kWave;        // one wave per slot
constexpr int kCdnMaskBytesPerThread = 16;
constexpr int kCdnMaskBytesPerBlock = kBlock * kCdnMaskBytesPerThread;
constexpr int64_t kCdnListLdsBytes = 60 * 1024;         // longest LDS slot list (below the 64 KiB default limit)

struct CdnArgs {
    const float *boxes;      // [B * capacity, 4]
    const int *labels;       // [B * capacity]
    const int *offsets;      // [B + 1]
    const float *weight;     // [C, E]
    const float *noise;      // [2 * groups, B * capacity, 10] (null: both noises off)
    int capacity, batch, max_gt, groups, num_classes, embed_dim, n_dn, total;   // total = n_dn + num_queries
    int row_blocks;
    float flip_threshold;    // label_noise_prob * 0.5 (<= 0: labels are kept)
    float box_noise_scale;
    float *label_queries;    // [B, n_dn, E]
    float *box_queries;      // [B, n_dn, 4]
    int *noised_labels;      // [B, n_dn]
    uint8_t *attn_mask;      // [total, total]
};

// util/misc.py:31-35
__device__ __forceinline__ float cdn_inverse_sigmoid(float x)
{
    x = fminf(fmaxf(x, 0.f), 1.f);
    const float x1 = fmaxf(x, 1e-3f);
    const float x2 = fmaxf(__fsub_rn(1.f, x), 1e-3f);
    return logf(__fdiv_rn(x1, x2));
}

__device__ __forceinline__ bool cdn_blocked(int i, int j, int n_dn, int group_slots)
{
    if (j >= n_dn) return false;
    return !(i < n_dn && i / group_slots == j / group_slots);
}

__global__ void __launch_bounds__(kBlock) cdn_queries_kernel(CdnArgs a)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if ((int)blockIdx.x >= a.row_blocks) {
        // ---- attention mask: 16 bytes per thread --------------------------------------------------------------
        const int64_t bytes = (int64_t)a.total * a.total;
        const int64_t first = ((int64_t)(blockIdx.x - a.row_blocks) * kBlock + tid) * kCdnMaskBytesPerThread;
        if (first >= bytes) return;
        const int group_slots = 2 * a.max_gt;
        int i = (int)(first / a.total), j = (int)(first - (int64_t)i * a.total);
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        const int n = (int)min((int64_t)kCdnMaskBytesPerThread, bytes - first);
        for (int k = 0; k < n; ++k) {
            if (cdn_blocked(i, j, a.n_dn, group_slots)) w[k >> 2] |= 1u << (8 * (k & 3));
            if (++j == a.total) {
                j = 0;
                ++i;
            }
        }
        if (n == kCdnMaskBytesPerThread) {
            *reinterpret_cast<uint4 *>(a.attn_mask + first) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            for (int k = 0; k < n; ++k) a.attn_mask[first + k] = (uint8_t)((w[k >> 2] >> (8 * (k & 3))) & 0xffu);
        }
        return;
    }
    // ---- one wave per slot ------------------------------------------------------------------------------------
    const int64_t slot = (int64_t)blockIdx.x * kCdnRowsPerBlock + wave;
    if (slot >= (int64_t)a.batch * a.n_dn) return;
    const int b = (int)(slot / a.n_dn), s = (int)(slot - (int64_t)b * a.n_dn);
    const int r = s / a.max_gt, t = s - r * a.max_gt;
    const int begin = a.offsets[b], count = a.offsets[b + 1] - begin;
    const int64_t staged_rows = (int64_t)a.batch * a.capacity;
    const int64_t src = (int64_t)begin + t;
    bool valid = t < count && begin >= 0 && src < staged_rows;
    int label = -1;
    const float *u = nullptr;
    if (valid) {
        label = a.labels[src];
        if (a.noise) u = a.noise + ((int64_t)r * staged_rows + src) * 10;
        if (a.flip_threshold > 0.f && u[0] < a.flip_threshold)
            label = min((int)floorf(__fmul_rn(u[1], (float)a.num_classes)), a.num_classes - 1);
        valid = label >= 0 && label < a.num_classes;
        if (!valid) label = -1;
    }
    float4 *out_row = reinterpret_cast<float4 *>(a.label_queries + slot * a.embed_dim);
    const int quads = a.embed_dim >> 2;
    if (valid) {
        const float4 *w_row = reinterpret_cast<const float4 *>(a.weight + (int64_t)label * a.embed_dim);
        for (int c = lane; c < quads; c += kWave) out_row[c] = w_row[c];
    } else {
        for (int c = lane; c < quads; c += kWave) out_row[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (lane != 0) return;
    a.noised_labels[slot] = label;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (valid) {
        const float4 bx = reinterpret_cast<const float4 *>(a.boxes)[src];
        float cx = bx.x, cy = bx.y, w = bx.z, h = bx.w;
        if (a.box_noise_scale > 0.f) {
            const float hw = __fdiv_rn(w, 2.f), hh = __fdiv_rn(h, 2.f);
            const float diff[4] = {hw, hh, hw, hh};
            float xyxy[4] = {__fsub_rn(cx, __fmul_rn(0.5f, w)), __fsub_rn(cy, __fmul_rn(0.5f, h)),
                             __fadd_rn(cx, __fmul_rn(0.5f, w)), __fadd_rn(cy, __fmul_rn(0.5f, h))};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float sign = __fsub_rn(__fmul_rn(u[2 + k] >= 0.5f ? 1.f : 0.f, 2.f), 1.f);
                float part = u[6 + k];
                if (r & 1) part = __fadd_rn(part, 1.f);
                part = __fmul_rn(part, sign);
                const float v = __fadd_rn(xyxy[k], __fmul_rn(__fmul_rn(part, diff[k]), a.box_noise_scale));
                xyxy[k] = fminf(fmaxf(v, 0.f), 1.f);
            }
            cx = __fdiv_rn(__fadd_rn(xyxy[0], xyxy[2]), 2.f);
            cy = __fdiv_rn(__fadd_rn(xyxy[1], xyxy[3]), 2.f);
            w = __fsub_rn(xyxy[2], xyxy[0]);
            h = __fsub_rn(xyxy[3], xyxy[1]);
        }
        q = make_float4(cdn_inverse_sigmoid(cx), cdn_inverse_sigmoid(cy), cdn_inverse_sigmoid(w), cdn_inverse_sigmoid(h));
    }
    reinterpret_cast<float4 *>(a.box_queries)[slot] = q;
}

template <bool LDS_LIST>
__global__ void __launch_bounds__(kBlock) cdn_label_grad_kernel(const float *__restrict__ grad, const int *__restrict__ labels,
                                                                int slots, int embed_dim, float *__restrict__ out)
{
    extern __shared__ __align__(16) int cdn_list[];
    __shared__ int n_match;
    const int cls = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    float *out_row = out + (int64_t)cls * embed_dim;
    if constexpr (LDS_LIST) {
        if (tid < kWave) {
            int n = 0;
            for (int base = 0; base < slots; base += kWave) {
                const int i = base + lane;
                const bool m = i < slots && labels[i] == cls;
                const uint64_t bal = __ballot(m);
                if (m) cdn_list[n + __popcll(bal & ((1ull << lane) - 1ull))] = i;
                n += __popcll(bal);
            }
            if (lane == 0) n_match = n;
        }
        __syncthreads();
        const int n = n_match;
        for (int col = tid; col < embed_dim; col += kBlock) {
            float acc = 0.f;
            for (int k = 0; k < n; ++k) acc = __fadd_rn(acc, grad[(int64_t)cdn_list[k] * embed_dim + col]);
            out_row[col] = acc;
        }
    } else {
        for (int col = tid; col < embed_dim; col += kBlock) {
            float acc = 0.f;
            for (int i = 0; i < slots; ++i)
                if (labels[i] == cls) acc = __fadd_rn(acc, grad[(int64_t)i * embed_dim + col]);
            out_row[col] = acc;
        }
    }
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace
}  // namespace sdetr

using namespace sdetr;

extern "C" int sdetr_cdn_queries(sdetr_stream_t stream, const float *boxes, const int *labels, const int *offsets,
                                 int capacity, const float *weight, const float *noise, int batch, int max_gt, int groups,
                                 int num_classes, int embed_dim, int num_queries, float label_noise_prob,
                                 float box_noise_scale, float *label_queries, float *box_queries, int *noised_labels,
                                 uint8_t *attn_mask)
{
    if (batch < 1 || capacity < 1 || num_classes < 1 || embed_dim < 1 || num_queries < 0)
        return fail("cdn_queries: bad sizes (batch %d, capacity %d, num_classes %d, embed_dim %d, num_queries %d)", batch,
                    capacity, num_classes, embed_dim, num_queries);
    if (groups < 1) return fail("cdn_queries: groups = %d, at least 1 expected", groups);
    if (max_gt < 1 || max_gt > capacity)
        return fail("cdn_queries: max_gt = %d outside [1, capacity = %d]", max_gt, capacity);
    if (embed_dim % 4 != 0) return fail("cdn_queries: embed_dim = %d is not a multiple of 4", embed_dim);
    const int64_t n_dn = 2 * (int64_t)groups * max_gt, total = n_dn + num_queries;
    if (total > 46340 || (int64_t)batch * n_dn > INT32_MAX / 4 || (int64_t)batch * capacity > INT32_MAX / 4)
        return fail("cdn_queries: n_dn + num_queries = %lld overflows (at most 46340 queries, 2^29 slots)", (long long)total);
    const bool any_noise = label_noise_prob > 0.f || box_noise_scale > 0.f;
    if (!boxes || !labels || !offsets || !weight || (any_noise && !noise) || !label_queries || !box_queries ||
        !noised_labels || !attn_mask)
        return fail("cdn_queries: null pointer");
    if (!aligned16(boxes) || !aligned16(weight) || !aligned16(label_queries) || !aligned16(box_queries) ||
        !aligned16(attn_mask))
        return fail("cdn_queries: boxes, weight, label_queries, box_queries and attn_mask must be 16-byte aligned");
    CdnArgs a{};
    a.boxes = boxes; a.labels = labels; a.offsets = offsets; a.weight = weight; a.noise = any_noise ? noise : nullptr;
    a.capacity = capacity; a.batch = batch; a.max_gt = max_gt; a.groups = groups; a.num_classes = num_classes;
    a.embed_dim = embed_dim; a.n_dn = (int)n_dn; a.total = (int)total;
    a.flip_threshold = label_noise_prob > 0.f ? label_noise_prob * 0.5f : 0.f;
    a.box_noise_scale = box_noise_scale;
    a.label_queries = label_queries; a.box_queries = box_queries; a.noised_labels = noised_labels; a.attn_mask = attn_mask;
    const int64_t rows = (int64_t)batch * n_dn;
    a.row_blocks = (int)((rows + kCdnRowsPerBlock - 1) / kCdnRowsPerBlock);
    const int64_t mask_blocks = (total * total + kCdnMaskBytesPerBlock - 1) / kCdnMaskBytesPerBlock;
    hipLaunchKernelGGL(cdn_queries_kernel, dim3((unsigned)(a.row_blocks + mask_blocks)), dim3(kBlock), 0,
                       (hipStream_t)stream, a);
    return check_launch("cdn_queries");
}

extern "C" int sdetr_cdn_label_grad(sdetr_stream_t stream, const float *grad_label_queries, const int *noised_labels,
                                    int batch, int n_dn, int num_classes, int embed_dim, float *grad_weight)
{
    if (batch < 1 || n_dn < 1 || num_classes < 1 || embed_dim < 1)
        return fail("cdn_label_grad: bad sizes (batch %d, n_dn %d, num_classes %d, embed_dim %d)", batch, n_dn,
                    num_classes, embed_dim);
    const int64_t slots = (int64_t)batch * n_dn;
    if (slots > INT32_MAX / 4) return fail("cdn_label_grad: batch * n_dn = %lld overflows", (long long)slots);
    if (!grad_label_queries || !noised_labels || !grad_weight) return fail("cdn_label_grad: null pointer");
    const int64_t lds = slots * 4;
    if (lds <= kCdnListLdsBytes)
        hipLaunchKernelGGL(cdn_label_grad_kernel<true>, dim3(num_classes), dim3(kBlock), (size_t)lds, (hipStream_t)stream,
                           grad_label_queries, noised_labels, (int)slots, embed_dim, grad_weight);
    else
        hipLaunchKernelGGL(cdn_label_grad_kernel<false>, dim3(num_classes), dim3(kBlock), 0, (hipStream_t)stream,
                           grad_label_queries, noised_labels, (int)slots, embed_dim, grad_weight);
    return check_launch("cdn_label_grad");
}

// The detector's set criterion (row N6): HybridSetCriterion with HungarianMatcher (reference
// models/bricks/set_criterion.py, models/matcher/hungarian_matcher.py, models/bricks/losses.py:15-22), device-resident.
//
//  * set_cost_kernel: the matcher's cost of every (output, image) problem, target-major [problem, T_cap, Nq] fp32:
//    2 * focal class cost + 5 * L1 cdist + 2 * (-GIoU) (weights are arguments), each operation rounded on its own as the
//    torch composite does.
//  * set_assign_kernel: exact minimum-cost rectangular assignment, one wavefront (= one workgroup) per problem.
//    Shortest augmenting paths (Crouse 2016, the algorithm of scipy's linear_sum_assignment without any initialisation
//    heuristic): targets are the augmenting rows, queries the columns, duals and path lengths in fp64.  Column state
//    (v, path length, predecessor, owner, scanned flag) lives in LDS, ~Nq / 64 columns per lane; the argmin of a step is
//    a 6-step shuffle reduction over (length, column is free, column index), the column index breaking ties.
//  * set_dn_match_kernel: the denoising loss's fixed assignment (models/detectors/base_detector.py:205-218),
//    query g * max_gt + t <-> target t.
//  * set_loss_kernel + set_loss_finish_kernel: vari_sigmoid_focal_loss with the matched IoU as target score, the L1 and the
//    GIoU box losses of every output: per-block partial sums in fp64, then a fixed-order sum per output (deterministic),
//    divided by num_boxes (a device scalar, never read by the host).
//  * set_loss_grad_kernel: d/dlogits (weight and target detached, as in the reference) and d/dboxes (L1 sign + the
//    analytic GIoU gradient through the cxcywh -> xyxy conversion, torch's clamp / min / max rules) of all outputs.
#include "common.h"

#pragma clang fp contract(off)

namespace sdetr {

constexpr int kSetMaxOutputs = 16;
constexpr int kSetThreads = 256;
constexpr int kSetPerThread = 8;
constexpr int kSetChunk = kSetThreads * kSetPerThread;  // logit elements per loss block
constexpr int kSetMaxLds = 64 * 1024;

enum SetStatus { kSetOk = 0, kSetTooManyTargets = 1, kSetOverCapacity = 2, kSetInfeasible = 3 };

struct SetOutputs {
    const void *logits[kSetMaxOutputs];
    int64_t logits_stride[kSetMaxOutputs];  // elements between images; queries num_classes apart
    const float *boxes[kSetMaxOutputs];
    int64_t boxes_stride[kSetMaxOutputs];   // floats between images; queries 4 apart
    int binary[kSetMaxOutputs];
    void *grad_logits[kSetMaxOutputs];      // backward: [B, Nq, C] contiguous, the logits' type
    float *grad_boxes[kSetMaxOutputs];      // backward: [B, Nq, 4] contiguous
};

struct SetTargets {
    const float *boxes;   // [sum T, 4] cxcywh
    const int *labels;    // [sum T]
    const int *offsets;   // [B + 1]
    int t_cap;
};

template <bool F16>
__device__ __forceinline__ float set_logit(const void *base, int64_t i)
{
    return F16 ? act_lo((uint32_t) reinterpret_cast<const uint16_t *>(base)[i]) : reinterpret_cast<const float *>(base)[i];
}

__device__ __forceinline__ float4 cxcywh_to_xyxy(float4 b)
{
    return make_float4(b.x - 0.5f * b.z, b.y - 0.5f * b.w, b.x + 0.5f * b.z, b.y + 0.5f * b.w);
}

// torchvision box_iou / generalized_box_iou on one pair, fp32, operations in torchvision's order
__device__ __forceinline__ void pair_iou(float4 a, float4 b, float &iou, float &giou)
{
    const float area_a = (a.z - a.x) * (a.w - a.y);
    const float area_b = (b.z - b.x) * (b.w - b.y);
    const float iw = fmaxf(fminf(a.z, b.z) - fmaxf(a.x, b.x), 0.f);
    const float ih = fmaxf(fminf(a.w, b.w) - fmaxf(a.y, b.y), 0.f);
    const float inter = iw * ih;
    const float uni = area_a + area_b - inter;
    iou = inter / uni;
    const float ew = fmaxf(fmaxf(a.z, b.z) - fminf(a.x, b.x), 0.f);
    const float eh = fmaxf(fmaxf(a.w, b.w) - fminf(a.y, b.y), 0.f);
    const float area_c = ew * eh;
    giou = iou - (area_c - uni) / area_c;
}

__device__ __forceinline__ float focal_pow(float v, float gamma) { return gamma == 2.f ? v * v : powf(v, gamma); }

// ---------------------------------------------------------------------------------------------------------------------
// cost
// ---------------------------------------------------------------------------------------------------------------------
struct CostArgs {
    SetOutputs out;
    SetTargets tg;
    int batch, nq, nc;
    float w_class, w_bbox, w_giou, alpha, gamma;
    float *cost;  // [problem, t_cap, nq]
};

template <bool F16>
__global__ void __launch_bounds__(kSetThreads) set_cost_kernel(CostArgs p)
{
    const int q = blockIdx.x * kSetThreads + threadIdx.x;
    const int t = blockIdx.y;
    const int prob = blockIdx.z;
    const int o = prob / p.batch, b = prob - o * p.batch;
    const int t0 = p.tg.offsets[b], nt = p.tg.offsets[b + 1] - t0;
    if (q >= p.nq || t >= nt || t >= p.tg.t_cap || nt > p.nq) return;
    const int label = p.out.binary[o] ? 0 : p.tg.labels[t0 + t];
    const float4 tb = reinterpret_cast<const float4 *>(p.tg.boxes)[t0 + t];
    const float4 qb = *reinterpret_cast<const float4 *>(p.out.boxes[o] + b * p.out.boxes_stride[o] + (int64_t)q * 4);
    float cls = 0.f;
    if (label >= 0 && label < p.nc) {
        const float x = set_logit<F16>(p.out.logits[o], b * p.out.logits_stride[o] + (int64_t)q * p.nc + label);
        const float prob_ = 1.f / (1.f + expf(-x));
        const float neg = -(1.f - p.alpha) * focal_pow(prob_, p.gamma) * logf(1.f - prob_ + 1e-6f);
        const float pos = -p.alpha * focal_pow(1.f - prob_, p.gamma) * logf(prob_ + 1e-6f);
        cls = pos - neg;
    }
    const float l1 = ((fabsf(qb.x - tb.x) + fabsf(qb.y - tb.y)) + fabsf(qb.z - tb.z)) + fabsf(qb.w - tb.w);
    float iou, giou;
    pair_iou(cxcywh_to_xyxy(qb), cxcywh_to_xyxy(tb), iou, giou);
    const float c = (p.w_bbox * l1 + p.w_class * cls) + p.w_giou * (-giou);
    p.cost[((int64_t)prob * p.tg.t_cap + t) * p.nq + q] = c;
}

// ---------------------------------------------------------------------------------------------------------------------
// assignment: one wavefront per problem
// ---------------------------------------------------------------------------------------------------------------------
struct AssignArgs {
    const float *cost;
    const int *offsets;
    int batch, nq, t_cap;
    int *match;     // [problem, nq]
    double *duals;  // [problem, nq + t_cap] (v then u), nullable
    int *status;    // [problem], nullable
};

struct Best {
    double val;
    int taken;  // 0: column is free (preferred on ties), 1: owned by a row
    int col;
    int owner;
};

__device__ __forceinline__ bool better(const Best &a, const Best &b)
{
    if (a.val != b.val) return a.val < b.val;
    if (a.taken != b.taken) return a.taken < b.taken;
    return a.col < b.col;
}

__device__ __forceinline__ Best wave_best(Best m)
{
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        Best o;
        o.val = __shfl_xor(m.val, s);
        o.taken = __shfl_xor(m.taken, s);
        o.col = __shfl_xor(m.col, s);
        o.owner = __shfl_xor(m.owner, s);
        if (better(o, m)) m = o;
    }
    return m;
}

__global__ void __launch_bounds__(64) set_assign_kernel(AssignArgs p)
{
    extern __shared__ double set_lds[];
    const int prob = blockIdx.x, lane = threadIdx.x;
    const int b = prob % p.batch;
    const int nq = p.nq;
    const int nt = p.offsets[b + 1] - p.offsets[b];
    int *match = p.match + (int64_t)prob * nq;
    double *v = set_lds;                      // [nq]
    double *spc = v + nq;                     // [nq]
    double *u = spc + nq;                     // [t_cap]
    int *path = reinterpret_cast<int *>(u + p.t_cap);  // [nq]
    int *row4col = path + nq;                 // [nq]
    int *col4row = row4col + nq;              // [t_cap]
    unsigned char *sc = reinterpret_cast<unsigned char *>(col4row + p.t_cap);  // [nq]
    unsigned char *sr = sc + nq;              // [t_cap]
    int status = kSetOk;
    if (nt > nq) status = kSetTooManyTargets;
    else if (nt > p.t_cap) status = kSetOverCapacity;
    const int T = status == kSetOk ? nt : 0;

    for (int j = lane; j < nq; j += 64) { v[j] = 0.0; row4col[j] = -1; }
    for (int i = lane; i < p.t_cap; i += 64) { u[i] = 0.0; col4row[i] = -1; }
    __syncthreads();

    const double inf = __builtin_huge_val();
    for (int cur = 0; cur < T && status == kSetOk; ++cur) {
        for (int j = lane; j < nq; j += 64) { spc[j] = inf; sc[j] = 0; }
        for (int i = lane; i < T; i += 64) sr[i] = 0;
        __syncthreads();
        double min_val = 0.0;
        int i = cur, sink = -1;
        while (sink < 0) {
            const double ui = u[i];
            const float *row = p.cost + ((int64_t)prob * p.t_cap + i) * nq;
            Best m{inf, 2, 0x7fffffff, -1};
            for (int j = lane; j < nq; j += 64) {
                if (sc[j]) continue;
                const double r = min_val + (double)row[j] - ui - v[j];
                double s = spc[j];
                if (r < s) { path[j] = i; spc[j] = r; s = r; }
                const int owner = row4col[j];
                const Best c{s, owner >= 0 ? 1 : 0, j, owner};
                if (better(c, m)) m = c;
            }
            m = wave_best(m);
            if (lane == 0) { sr[i] = 1; if (m.col < nq) sc[m.col] = 1; }
            __syncthreads();
            if (m.col >= nq || !(m.val < inf)) { status = kSetInfeasible; break; }  // NaN / inf costs
            min_val = m.val;
            if (m.taken) i = m.owner;
            else sink = m.col;
        }
        if (status != kSetOk) break;
        // duals (scipy's order: before the augmentation, with the old col4row)
        for (int r = lane; r < T; r += 64)
            if (sr[r]) u[r] += r == cur ? min_val : min_val - spc[col4row[r]];
        for (int j = lane; j < nq; j += 64)
            if (sc[j]) v[j] -= min_val - spc[j];
        __syncthreads();
        if (lane == 0) {
            int j = sink;
            for (;;) {
                const int r = path[j];
                row4col[j] = r;
                const int prev = col4row[r];
                col4row[r] = j;
                j = prev;
                if (r == cur) break;
            }
        }
        __syncthreads();
    }
    for (int j = lane; j < nq; j += 64) match[j] = status == kSetOk ? row4col[j] : -1;
    if (p.duals) {
        double *d = p.duals + (int64_t)prob * (nq + p.t_cap);
        for (int j = lane; j < nq; j += 64) d[j] = status == kSetOk ? v[j] : 0.0;
        for (int r = lane; r < p.t_cap; r += 64) d[nq + r] = (status == kSetOk && r < T) ? u[r] : 0.0;
    }
    if (p.status && lane == 0) p.status[prob] = status;
}

// the denoising loss's assignment: query g * max_gt + t <-> target t, t < min(T, max_gt), g < groups
__global__ void __launch_bounds__(kSetThreads) set_dn_match_kernel(const int *offsets, int batch, int nq, int groups,
                                                                    int max_gt, int *match, int *status)
{
    const int q = blockIdx.x * kSetThreads + threadIdx.x;
    const int prob = blockIdx.y, b = prob % batch;
    const int nt = offsets[b + 1] - offsets[b];
    if (q < nq) {
        const int g = q / max_gt, t = q - g * max_gt;
        match[(int64_t)prob * nq + q] = (g < groups && t < nt) ? t : -1;
    }
    if (status && q == 0) status[prob] = nt > max_gt ? kSetOverCapacity : kSetOk;
}

// ---------------------------------------------------------------------------------------------------------------------
// losses
// ---------------------------------------------------------------------------------------------------------------------
struct LossArgs2 {
    SetOutputs out;
    SetTargets tg;
    int batch, nq, nc, chunks;
    const int *match;          // [n_outputs * batch, nq]
    const float *num_boxes;    // device scalar or null (= max(offsets[B], 1))
    float num_boxes_scale;
    float alpha, gamma;
    double *partial;           // [n_outputs, batch, chunks, 3]
    const float *grad_losses;  // backward: [n_outputs, 3]
};

__device__ __forceinline__ float set_num_boxes(const LossArgs2 &p)
{
    const float nb = p.num_boxes ? p.num_boxes[0] : fmaxf((float)p.tg.offsets[p.batch], 1.f);
    return nb * p.num_boxes_scale;
}

// one logit's share of vari_sigmoid_focal_loss: weight * BCE-with-logits, and d/dx of it (weight, target detached)
__device__ __forceinline__ void vari_focal(float x, float onehot, float score, float alpha, float gamma, float &loss,
                                           float &dx)
{
    const float prob = 1.f / (1.f + expf(-x));
    const float target = onehot * score;
    const float w = (1.f - alpha) * focal_pow(prob, gamma) * (1.f - onehot) + target;
    const float bce = (1.f - target) * x + (fmaxf(-x, 0.f) + log1pf(expf(-fabsf(x))));
    loss = bce * w;
    dx = w * (prob - target);
}

__device__ __forceinline__ double block_sum_d(double v, double *scratch)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
    __syncthreads();
    return r;
}

template <bool F16>
__global__ void __launch_bounds__(kSetThreads) set_loss_kernel(LossArgs2 p)
{
    __shared__ double scratch[4];
    const int chunk = blockIdx.x, b = blockIdx.y, o = blockIdx.z;
    const int t0 = p.tg.offsets[b];
    const int *match = p.match + ((int64_t)o * p.batch + b) * p.nq;
    const int64_t n = (int64_t)p.nq * p.nc;
    const void *logits = p.out.logits[o];
    const int64_t lbase = b * p.out.logits_stride[o];
    const float *boxes = p.out.boxes[o] + b * p.out.boxes_stride[o];
    float cls = 0.f, l1 = 0.f, lg = 0.f;
#pragma unroll
    for (int k = 0; k < kSetPerThread; ++k) {
        const int64_t e = (int64_t)chunk * kSetChunk + k * kSetThreads + threadIdx.x;
        if (e >= n) break;
        const int q = (int)(e / p.nc), c = (int)(e - (int64_t)q * p.nc);
        const int t = match[q];
        float onehot = 0.f, score = 0.f;
        if (t >= 0) {
            const int label = p.out.binary[o] ? 0 : p.tg.labels[t0 + t];
            const float4 qb = cxcywh_to_xyxy(*reinterpret_cast<const float4 *>(boxes + (int64_t)q * 4));
            const float4 tbc = reinterpret_cast<const float4 *>(p.tg.boxes)[t0 + t];
            const float4 tb = cxcywh_to_xyxy(tbc);
            float iou, giou;
            pair_iou(qb, tb, iou, giou);
            if (c == label) { onehot = 1.f; score = iou; }
            if (c == 0) {
                const float4 s = *reinterpret_cast<const float4 *>(boxes + (int64_t)q * 4);
                l1 += ((fabsf(s.x - tbc.x) + fabsf(s.y - tbc.y)) + fabsf(s.z - tbc.z)) + fabsf(s.w - tbc.w);
                lg += 1.f - giou;
            }
        }
        float l, d;
        vari_focal(set_logit<F16>(logits, lbase + e), onehot, score, p.alpha, p.gamma, l, d);
        cls += l;
    }
    const double s0 = block_sum_d((double)cls, scratch);
    const double s1 = block_sum_d((double)l1, scratch);
    const double s2 = block_sum_d((double)lg, scratch);
    if (threadIdx.x == 0) {
        double *dst = p.partial + (((int64_t)o * p.batch + b) * p.chunks + chunk) * 3;
        dst[0] = s0; dst[1] = s1; dst[2] = s2;
    }
}

__global__ void __launch_bounds__(kSetThreads) set_loss_finish_kernel(LossArgs2 p, float *losses)
{
    __shared__ double scratch[4];
    const int o = blockIdx.x;
    const int per = p.batch * p.chunks;
    const double *src = p.partial + (int64_t)o * per * 3;
    double a[3] = {0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < per; i += kSetThreads)
        for (int k = 0; k < 3; ++k) a[k] += src[(int64_t)i * 3 + k];
    const float nb = set_num_boxes(p);
    for (int k = 0; k < 3; ++k) {
        const double s = block_sum_d(a[k], scratch);
        if (threadIdx.x == 0) losses[o * 3 + k] = (float)(s / (double)nb);
    }
}

// d giou(a, b) / d a for a, b in xyxy, torch's rules: clamp(min=0) passes the gradient where its input >= 0,
// torch.min / torch.max of two tensors split it in half on a tie
__device__ __forceinline__ double tie_share(float a, float b, bool a_wins) { return a == b ? 0.5 : (a_wins ? 1.0 : 0.0); }

__device__ void giou_grad(float4 af, float4 bf, double g, double da[4])
{
    const double ax0 = af.x, ay0 = af.y, ax1 = af.z, ay1 = af.w;
    const double bx0 = bf.x, by0 = bf.y, bx1 = bf.z, by1 = bf.w;
    const double area_a = (ax1 - ax0) * (ay1 - ay0), area_b = (bx1 - bx0) * (by1 - by0);
    const double iw_raw = fmin(ax1, bx1) - fmax(ax0, bx0), ih_raw = fmin(ay1, by1) - fmax(ay0, by0);
    const double iw = fmax(iw_raw, 0.0), ih = fmax(ih_raw, 0.0);
    const double inter = iw * ih;
    const double uni = area_a + area_b - inter;
    const double ew_raw = fmax(ax1, bx1) - fmin(ax0, bx0), eh_raw = fmax(ay1, by1) - fmin(ay0, by0);
    const double ew = fmax(ew_raw, 0.0), eh = fmax(eh_raw, 0.0);
    const double area_c = ew * eh;
    // giou = inter / uni - (area_c - uni) / area_c
    const double d_c = g * (-uni / (area_c * area_c));
    const double d_uni = g * (-inter / (uni * uni) + 1.0 / area_c);
    const double d_inter = g / uni - d_uni;
    const double d_area_a = d_uni;
    const double d_iw = iw_raw >= 0.0 ? d_inter * ih : 0.0, d_ih = ih_raw >= 0.0 ? d_inter * iw : 0.0;
    const double d_ew = ew_raw >= 0.0 ? d_c * eh : 0.0, d_eh = eh_raw >= 0.0 ? d_c * ew : 0.0;
    double dx0 = 0, dy0 = 0, dx1 = 0, dy1 = 0;
    // iw = min(ax1, bx1) - max(ax0, bx0);  ew = max(ax1, bx1) - min(ax0, bx0)
    dx1 += d_iw * tie_share(af.z, bf.z, af.z < bf.z) + d_ew * tie_share(af.z, bf.z, af.z > bf.z);
    dx0 += -d_iw * tie_share(af.x, bf.x, af.x > bf.x) - d_ew * tie_share(af.x, bf.x, af.x < bf.x);
    dy1 += d_ih * tie_share(af.w, bf.w, af.w < bf.w) + d_eh * tie_share(af.w, bf.w, af.w > bf.w);
    dy0 += -d_ih * tie_share(af.y, bf.y, af.y > bf.y) - d_eh * tie_share(af.y, bf.y, af.y < bf.y);
    dx1 += d_area_a * (ay1 - ay0); dx0 -= d_area_a * (ay1 - ay0);
    dy1 += d_area_a * (ax1 - ax0); dy0 -= d_area_a * (ax1 - ax0);
    da[0] = dx0; da[1] = dy0; da[2] = dx1; da[3] = dy1;
}

__device__ __forceinline__ float l1_sign(float a, float b) { return a > b ? 1.f : (a < b ? -1.f : 0.f); }

template <bool F16>
__global__ void __launch_bounds__(kSetThreads) set_loss_grad_kernel(LossArgs2 p)
{
    const int chunk = blockIdx.x, b = blockIdx.y, o = blockIdx.z;
    const int t0 = p.tg.offsets[b];
    const int *match = p.match + ((int64_t)o * p.batch + b) * p.nq;
    const int64_t n = (int64_t)p.nq * p.nc;
    const void *logits = p.out.logits[o];
    const int64_t lbase = b * p.out.logits_stride[o];
    const float *boxes = p.out.boxes[o] + b * p.out.boxes_stride[o];
    const float nb = set_num_boxes(p);
    const float g_cls = p.grad_losses[o * 3 + 0] / nb;
    const float g_l1 = p.grad_losses[o * 3 + 1] / nb;
    const double g_giou = (double)p.grad_losses[o * 3 + 2] / (double)nb;
    float *gbox = p.out.grad_boxes[o] + (int64_t)b * p.nq * 4;
#pragma unroll
    for (int k = 0; k < kSetPerThread; ++k) {
        const int64_t e = (int64_t)chunk * kSetChunk + k * kSetThreads + threadIdx.x;
        if (e >= n) break;
        const int q = (int)(e / p.nc), c = (int)(e - (int64_t)q * p.nc);
        const int t = match[q];
        float onehot = 0.f, score = 0.f;
        float4 gq = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t >= 0) {
            const int label = p.out.binary[o] ? 0 : p.tg.labels[t0 + t];
            const float4 s = *reinterpret_cast<const float4 *>(boxes + (int64_t)q * 4);
            const float4 tbc = reinterpret_cast<const float4 *>(p.tg.boxes)[t0 + t];
            const float4 qb = cxcywh_to_xyxy(s), tb = cxcywh_to_xyxy(tbc);
            float iou, giou;
            pair_iou(qb, tb, iou, giou);
            if (c == label) { onehot = 1.f; score = iou; }
            if (c == 0) {
                double da[4];
                giou_grad(qb, tb, -g_giou, da);  // loss = 1 - giou
                // x0 = cx - 0.5 w, x1 = cx + 0.5 w
                gq.x = l1_sign(s.x, tbc.x) * g_l1 + (float)(da[0] + da[2]);
                gq.y = l1_sign(s.y, tbc.y) * g_l1 + (float)(da[1] + da[3]);
                gq.z = l1_sign(s.z, tbc.z) * g_l1 + (float)(0.5 * (da[2] - da[0]));
                gq.w = l1_sign(s.w, tbc.w) * g_l1 + (float)(0.5 * (da[3] - da[1]));
            }
        }
        if (c == 0) reinterpret_cast<float4 *>(gbox)[q] = gq;
        float l, d;
        vari_focal(set_logit<F16>(logits, lbase + e), onehot, score, p.alpha, p.gamma, l, d);
        const float gx = d * g_cls;
        if (F16) reinterpret_cast<uint16_t *>(p.out.grad_logits[o])[(int64_t)b * n + e] = (uint16_t)f32_to_act_bits(gx);
        else reinterpret_cast<float *>(p.out.grad_logits[o])[(int64_t)b * n + e] = gx;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------------
static size_t assign_lds_bytes(int nq, int t_cap)
{
    return (size_t)(2 * nq + t_cap) * 8 + (size_t)(2 * nq + t_cap) * 4 + (size_t)nq + (size_t)t_cap;
}

static int fill_outputs(const char *what, const sdetr_set_output *outputs, int n_outputs, int batch, int nq, int nc,
                        bool need_logits, SetOutputs &o)
{
    if (n_outputs < 1 || n_outputs > kSetMaxOutputs) return fail("%s: %d outputs (1..%d)", what, n_outputs, kSetMaxOutputs);
    if (!outputs) return fail("%s: null output table", what);
    for (int i = 0; i < n_outputs; ++i) {
        const sdetr_set_output &s = outputs[i];
        if ((need_logits && !s.logits) || !s.boxes) return fail("%s: output %d has a null pointer", what, i);
        if (batch > 1 && s.logits_batch_stride < (int64_t)nq * nc)
            return fail("%s: output %d: logits batch stride smaller than num_queries * num_classes", what, i);
        if (batch > 1 && s.boxes_batch_stride < (int64_t)nq * 4)
            return fail("%s: output %d: boxes batch stride smaller than num_queries * 4", what, i);
        if ((reinterpret_cast<uintptr_t>(s.boxes) & 15) || (s.boxes_batch_stride & 3))
            return fail("%s: output %d: boxes must be 16-byte aligned, images a multiple of 4 floats apart", what, i);
        o.logits[i] = s.logits; o.logits_stride[i] = s.logits_batch_stride;
        o.boxes[i] = s.boxes; o.boxes_stride[i] = s.boxes_batch_stride; o.binary[i] = s.binary_cls ? 1 : 0;
        o.grad_logits[i] = nullptr; o.grad_boxes[i] = nullptr;
    }
    return 0;
}

static int check_targets(const char *what, const float *tgt_boxes, const int *tgt_labels, const int *tgt_offsets, int t_cap)
{
    if (!tgt_boxes || !tgt_labels || !tgt_offsets) return fail("%s: null target pointer", what);
    if (reinterpret_cast<uintptr_t>(tgt_boxes) & 15) return fail("%s: target boxes must be 16-byte aligned", what);
    if (t_cap < 0) return fail("%s: negative target capacity", what);
    return 0;
}

}  // namespace sdetr

using namespace sdetr;

extern "C" int64_t sdetr_set_match_workspace_bytes(int problems, int t_cap, int num_queries)
{
    if (problems < 0 || t_cap < 0 || num_queries < 0) return -1;
    return (int64_t)problems * t_cap * num_queries * (int64_t)sizeof(float);
}

extern "C" int sdetr_set_match(sdetr_stream_t stream, const sdetr_set_output *outputs, int n_outputs, int logits_dtype,
                               int batch, int num_queries, int num_classes, const float *tgt_boxes, const int *tgt_labels,
                               const int *tgt_offsets, int t_cap, float cost_class, float cost_bbox, float cost_giou,
                               float focal_alpha, float focal_gamma, int dn_groups, int dn_max_gt, void *workspace,
                               int64_t workspace_bytes, int *match, double *duals, int *status)
{
    const char *what = "set_match";
    if (batch < 1 || num_queries < 1 || num_classes < 1 || n_outputs < 1 || n_outputs > kSetMaxOutputs)
        return fail("%s: bad sizes (batch %d, queries %d, classes %d, outputs %d)", what, batch, num_queries, num_classes,
                    n_outputs);
    if (!match || !tgt_offsets) return fail("%s: null pointer", what);
    const int problems = n_outputs * batch;
    hipStream_t s = (hipStream_t)stream;
    if (dn_groups > 0) {
        if (dn_max_gt < 1 || (int64_t)dn_groups * dn_max_gt > num_queries)
            return fail("%s: denoising groups %d x max targets %d do not fit %d queries", what, dn_groups, dn_max_gt,
                        num_queries);
        hipLaunchKernelGGL(set_dn_match_kernel, dim3((unsigned)((num_queries + kSetThreads - 1) / kSetThreads), problems),
                           dim3(kSetThreads), 0, s, tgt_offsets, batch, num_queries, dn_groups, dn_max_gt, match, status);
        return check_launch(what);
    }
    if (logits_dtype != SDETR_F32 && logits_dtype != kActCode)
        return fail("%s: logits dtype %d is neither f32 nor this library's 16-bit type", what, logits_dtype);
    if (int rc = check_targets(what, tgt_boxes, tgt_labels, tgt_offsets, t_cap)) return rc;
    if (t_cap > num_queries) return fail("%s: target capacity %d exceeds %d queries", what, t_cap, num_queries);
    if (t_cap > 65535) return fail("%s: target capacity %d above 65535", what, t_cap);
    const size_t lds = assign_lds_bytes(num_queries, t_cap);
    if (lds > (size_t)kSetMaxLds)
        return fail("%s: %d queries x %d targets need %zu bytes of LDS (> %d)", what, num_queries, t_cap, lds, kSetMaxLds);
    const int64_t need = sdetr_set_match_workspace_bytes(problems, t_cap, num_queries);
    if (need > 0 && (!workspace || workspace_bytes < need)) return fail("%s: workspace too small (%lld bytes needed)", what,
                                                                        (long long)need);
    CostArgs c{};
    if (int rc = fill_outputs(what, outputs, n_outputs, batch, num_queries, num_classes, true, c.out)) return rc;
    c.tg = SetTargets{tgt_boxes, tgt_labels, tgt_offsets, t_cap};
    c.batch = batch; c.nq = num_queries; c.nc = num_classes;
    c.w_class = cost_class; c.w_bbox = cost_bbox; c.w_giou = cost_giou; c.alpha = focal_alpha; c.gamma = focal_gamma;
    c.cost = (float *)workspace;
    if (t_cap > 0) {
        const dim3 grid((unsigned)((num_queries + kSetThreads - 1) / kSetThreads), (unsigned)t_cap, (unsigned)problems);
        if (logits_dtype == SDETR_F32) hipLaunchKernelGGL(set_cost_kernel<false>, grid, dim3(kSetThreads), 0, s, c);
        else hipLaunchKernelGGL(set_cost_kernel<true>, grid, dim3(kSetThreads), 0, s, c);
        if (int rc = check_launch("set_match (cost)")) return rc;
    }
    AssignArgs a{(const float *)workspace, tgt_offsets, batch, num_queries, t_cap, match, duals, status};
    hipLaunchKernelGGL(set_assign_kernel, dim3((unsigned)problems), dim3(64), lds, s, a);
    return check_launch("set_match (assign)");
}

static int set_loss_args(const char *what, const sdetr_set_output *outputs, int n_outputs, int logits_dtype, int batch,
                         int num_queries, int num_classes, const float *tgt_boxes, const int *tgt_labels,
                         const int *tgt_offsets, const int *match, const float *num_boxes, float num_boxes_scale,
                         float alpha, float gamma, LossArgs2 &a)
{
    if (batch < 1 || num_queries < 1 || num_classes < 1) return fail("%s: bad sizes", what);
    if ((int64_t)num_queries * num_classes > 0x7fffffff) return fail("%s: num_queries * num_classes above 2^31", what);
    if (logits_dtype != SDETR_F32 && logits_dtype != kActCode)
        return fail("%s: logits dtype %d is neither f32 nor this library's 16-bit type", what, logits_dtype);
    if (int rc = check_targets(what, tgt_boxes, tgt_labels, tgt_offsets, 0)) return rc;
    if (!match) return fail("%s: null match", what);
    if (!(num_boxes_scale > 0.f)) return fail("%s: num_boxes_scale must be > 0", what);
    if (int rc = fill_outputs(what, outputs, n_outputs, batch, num_queries, num_classes, true, a.out)) return rc;
    a.tg = SetTargets{tgt_boxes, tgt_labels, tgt_offsets, 0};
    a.batch = batch; a.nq = num_queries; a.nc = num_classes;
    a.chunks = (int)(((int64_t)num_queries * num_classes + kSetChunk - 1) / kSetChunk);
    a.match = match; a.num_boxes = num_boxes; a.num_boxes_scale = num_boxes_scale; a.alpha = alpha; a.gamma = gamma;
    return 0;
}

extern "C" int64_t sdetr_set_loss_workspace_bytes(int n_outputs, int batch, int num_queries, int num_classes)
{
    if (n_outputs < 0 || batch < 0 || num_queries < 0 || num_classes < 0) return -1;
    const int64_t chunks = ((int64_t)num_queries * num_classes + kSetChunk - 1) / kSetChunk;
    return (int64_t)n_outputs * batch * chunks * 3 * (int64_t)sizeof(double);
}

extern "C" int sdetr_set_loss(sdetr_stream_t stream, const sdetr_set_output *outputs, int n_outputs, int logits_dtype,
                              int batch, int num_queries, int num_classes, const float *tgt_boxes, const int *tgt_labels,
                              const int *tgt_offsets, const int *match, const float *num_boxes, float num_boxes_scale,
                              float alpha, float gamma, void *workspace, int64_t workspace_bytes, float *losses)
{
    LossArgs2 a{};
    if (int rc = set_loss_args("set_loss", outputs, n_outputs, logits_dtype, batch, num_queries, num_classes, tgt_boxes,
                               tgt_labels, tgt_offsets, match, num_boxes, num_boxes_scale, alpha, gamma, a))
        return rc;
    if (!losses) return fail("set_loss: null losses");
    const int64_t need = sdetr_set_loss_workspace_bytes(n_outputs, batch, num_queries, num_classes);
    if (!workspace || workspace_bytes < need) return fail("set_loss: workspace too small (%lld bytes needed)", (long long)need);
    a.partial = (double *)workspace;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)a.chunks, (unsigned)batch, (unsigned)n_outputs);
    if (logits_dtype == SDETR_F32) hipLaunchKernelGGL(set_loss_kernel<false>, grid, dim3(kSetThreads), 0, s, a);
    else hipLaunchKernelGGL(set_loss_kernel<true>, grid, dim3(kSetThreads), 0, s, a);
    if (int rc = check_launch("set_loss")) return rc;
    hipLaunchKernelGGL(set_loss_finish_kernel, dim3((unsigned)n_outputs), dim3(kSetThreads), 0, s, a, losses);
    return check_launch("set_loss (finish)");
}

extern "C" int sdetr_set_loss_backward(sdetr_stream_t stream, const sdetr_set_output *outputs, int n_outputs,
                                       int logits_dtype, int batch, int num_queries, int num_classes,
                                       const float *tgt_boxes, const int *tgt_labels, const int *tgt_offsets,
                                       const int *match, const float *num_boxes, float num_boxes_scale, float alpha,
                                       float gamma, const float *grad_losses, void *const *grad_logits,
                                       float *const *grad_boxes)
{
    LossArgs2 a{};
    if (int rc = set_loss_args("set_loss_backward", outputs, n_outputs, logits_dtype, batch, num_queries, num_classes,
                               tgt_boxes, tgt_labels, tgt_offsets, match, num_boxes, num_boxes_scale, alpha, gamma, a))
        return rc;
    if (!grad_losses || !grad_logits || !grad_boxes) return fail("set_loss_backward: null pointer");
    for (int i = 0; i < n_outputs; ++i) {
        if (!grad_logits[i] || !grad_boxes[i]) return fail("set_loss_backward: output %d has a null gradient", i);
        if (reinterpret_cast<uintptr_t>(grad_boxes[i]) & 15) return fail("set_loss_backward: grad_boxes must be 16-byte aligned");
        a.out.grad_logits[i] = grad_logits[i];
        a.out.grad_boxes[i] = grad_boxes[i];
    }
    a.grad_losses = grad_losses;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)a.chunks, (unsigned)batch, (unsigned)n_outputs);
    if (logits_dtype == SDETR_F32) hipLaunchKernelGGL(set_loss_grad_kernel<false>, grid, dim3(kSetThreads), 0, s, a);
    else hipLaunchKernelGGL(set_loss_grad_kernel<true>, grid, dim3(kSetThreads), 0, s, a);
    return check_launch("set_loss_backward");
}

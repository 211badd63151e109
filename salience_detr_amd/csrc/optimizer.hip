// The optimizer step of the training loop (reference util/engine.py:56-61): accelerator.clip_grad_norm_(parameters, 0.1)
// followed by torch.optim.AdamW.step(), as TWO launches over every parameter of the step.
//
// Addressing.  Parameters and gradients stay where their owners keep them; the two moments live in two flat fp32 buffers.
// Three small device tables describe the step:
//  * records [num_records]  (sdetr_adamw_record): parameter pointer, gradient pointer, offset of the tensor in the flat
//    moment buffers, length, parameter group, and `lag` = how many steps of the shared counter this tensor has NOT taken
//    (torch.optim.AdamW counts steps per parameter and skips one whose gradient is None);
//  * chunks [num_chunks]  (sdetr_adamw_chunk): (record, first element, count), count <= kAdamChunk = 1024 elements: what
//    one WAVE updates as 4 x 16 bytes per lane and stream;
//  * wave_first [num_waves + 1]: wave item w owns chunks wave_first[w] .. wave_first[w + 1] - 1.  A 2048 x 256 weight is
//    512 items of one full chunk each (128 workgroups); biases, norms and `alpha` are packed several to an item (up to
//    1024 elements together), so a tiny tensor costs a few lanes of one wave, not a workgroup.
//
// Launch 1, adamw_sumsq_kernel: num_partials (<= 1024) workgroups, each over a contiguous range of wave items; a lane adds
// g * g in double (the product of two floats is exact in double), lanes combine by a fixed butterfly, the four waves in
// wave order, and the workgroup writes ONE double to partials[block].  No atomics, no counter to clear, no memset: every
// partial is overwritten by every launch.  Thread 0 of workgroup 0 also advances the device step counter.
//
// Launch 2, adamw_update_kernel: one workgroup per four wave items.  Every workgroup adds the partials itself, in the same
// order (lane t takes partials t, t + 256, ..; the same butterfly; waves in order), so the norm is the same bit pattern in
// every workgroup: total_norm = float(grad_scale * sqrt(sum)), coef = min(1, max_norm / (total_norm + 1e-6)) as
// torch.nn.utils.clip_grad_norm_ forms it in fp32 (a NaN stays a NaN, as torch's clamp keeps it; max_norm <= 0: coef = 1),
// and g' = g * (grad_scale * coef).  Then torch.optim.AdamW's single-tensor statement, every operation rounded on its own
// in fp32 (no contraction), its scalars formed in double from the step counter as the Python side of torch forms them:
//     p  = p * (1 - lr * wd)
//     m  = m + (g' - m) * (1 - beta1)                                  (lerp_)
//     v  = v * beta2 + ((1 - beta2) * g') * g'                         (mul_, addcmul_)
//     p  = p + ((-lr / (1 - beta1^t)) * m) / (sqrt(v) / sqrt(1 - beta2^t) + eps)
// It writes p, m, v (never g) and, from workgroup 0, total_norm.  A non-finite norm makes the update non-finite
// (error_if_nonfinite=False); nothing traps.
//
// Vector width: a chunk starts with up to three single elements until the parameter address is 16-byte aligned, then
// moves float4 per lane while the moments are aligned there too (the host places a tensor's moments at the parameter's
// misalignment, so they are), then single elements again.  A gradient that is misaligned against its parameter (a slice
// of a flat all-reduce buffer behind an odd-sized tensor) is read as four dwords.  Roofline: 28 B per element in launch 2
// (read g, p, m, v; write p, m, v) + 4 B in launch 1.
#include "common.h"

#pragma clang fp contract(off)

namespace sdetr {
namespace {

constexpr int kAdamChunk = SDETR_ADAMW_CHUNK;                 // elements per chunk (one wave, 4 float4 per lane)
constexpr int kAdamMaxPartials = SDETR_ADAMW_MAX_PARTIALS;
constexpr int kAdamWaves = kBlock / kWave;

struct AdamTables {
    const sdetr_adamw_record *records;
    const sdetr_adamw_chunk *chunks;
    const int *wave_first;
    int num_records, num_chunks, num_waves, num_partials;
};

// lanes of a wave, fixed butterfly: every lane ends with the same bits
__device__ __forceinline__ double wave_sum(double x)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, kWave);
    return x;
}

// sum over the workgroup, waves added in wave order; every thread returns the same bits
__device__ __forceinline__ double block_sum(double x, double *lds)
{
    x = wave_sum(x);
    const int wave = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) lds[wave] = x;
    __syncthreads();
    double s = lds[0];
#pragma unroll
    for (int w = 1; w < kAdamWaves; ++w) s += lds[w];
    __syncthreads();
    return s;
}

// a chunk record checked against the tables (a bad table entry is skipped, never followed out of bounds)
__device__ __forceinline__ bool chunk_ok(const AdamTables &t, const sdetr_adamw_chunk &c)
{
    if (c.record < 0 || c.record >= t.num_records || c.start < 0 || c.count < 1 || c.count > kAdamChunk) return false;
    return (int64_t)c.start + c.count <= t.records[c.record].length;
}

__device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
__device__ __forceinline__ int to_aligned16(const float *p) { return (int)((4u - ((reinterpret_cast<uintptr_t>(p) >> 2) & 3u)) & 3u); }

__device__ __forceinline__ float4 load_gradient4(const float *g, bool aligned)
{
    if (aligned) return *reinterpret_cast<const float4 *>(g);
    return make_float4(g[0], g[1], g[2], g[3]);
}

__global__ void __launch_bounds__(kBlock) adamw_sumsq_kernel(AdamTables t, double *partials, int *step_counter)
{
    __shared__ double lds[kAdamWaves];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int per = (t.num_waves + t.num_partials - 1) / t.num_partials;
    const int item_begin = blockIdx.x * per, item_end = min(t.num_waves, item_begin + per);
    double acc = 0.0;
    for (int item = item_begin + wave; item < item_end; item += kAdamWaves) {
        for (int ci = t.wave_first[item]; ci < t.wave_first[item + 1] && ci < t.num_chunks; ++ci) {
            const sdetr_adamw_chunk c = t.chunks[ci];
            if (!chunk_ok(t, c)) continue;
            const float *g = t.records[c.record].grad + c.start;
            const int head = min(c.count, to_aligned16(g));
            const int body = (c.count - head) & ~3;
            if (lane < head) acc += (double)g[lane] * (double)g[lane];
            for (int i = head + lane * 4; i < head + body; i += kWave * 4) {
                const float4 x = *reinterpret_cast<const float4 *>(g + i);
                acc += (double)x.x * (double)x.x;
                acc += (double)x.y * (double)x.y;
                acc += (double)x.z * (double)x.z;
                acc += (double)x.w * (double)x.w;
            }
            const int i = head + body + lane;
            if (i < c.count) acc += (double)g[i] * (double)g[i];
        }
    }
    const double s = block_sum(acc, lds);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = s;
        if (blockIdx.x == 0) *step_counter = *step_counter + 1;
    }
}

struct AdamScalars {      // what one tensor's elements share
    float clip;           // grad_scale * coef
    float decay;          // 1 - lr * wd
    float lerp_weight;    // 1 - beta1
    float beta2, one_minus_beta2;
    float neg_step_size;  // -lr / (1 - beta1^t)
    float bc2_sqrt;       // sqrt(1 - beta2^t)
    float eps;
};

__device__ __forceinline__ void adamw_element(const AdamScalars &s, float g, float &p, float &m, float &v)
{
    g = g * s.clip;
    p = p * s.decay;
    m = m + (g - m) * s.lerp_weight;
    v = v * s.beta2 + (s.one_minus_beta2 * g) * g;
    const float denom = __fdiv_rn(__fsqrt_rn(v), s.bc2_sqrt) + s.eps;
    p = p + __fdiv_rn(s.neg_step_size * m, denom);
}

struct AdamHyper {
    const double *groups;     // [num_groups, 2]: lr, weight_decay
    int num_groups;
    double beta1, beta2, eps;
    float max_norm, grad_scale;
};

__global__ void __launch_bounds__(kBlock) adamw_update_kernel(AdamTables t, AdamHyper h, const double *partials,
                                                              const int *step_counter, float *exp_avg, float *exp_avg_sq,
                                                              float *norm_out)
{
    __shared__ double lds[kAdamWaves];
    __shared__ double shared_pow[2];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    double acc = 0.0;
    for (int i = threadIdx.x; i < t.num_partials; i += kBlock) acc += partials[i];
    const int step = *step_counter;
    if (threadIdx.x == 0) {       // beta^t of a tensor that has taken every step: once per workgroup
        shared_pow[0] = pow(h.beta1, (double)step);
        shared_pow[1] = pow(h.beta2, (double)step);
    }
    const double sumsq = block_sum(acc, lds);     // (its barriers publish shared_pow too)
    const float total_norm = (float)((double)h.grad_scale * sqrt(sumsq));
    float coef = 1.f;
    if (h.max_norm > 0.f) {
        coef = __fdiv_rn(h.max_norm, total_norm + 1e-6f);
        coef = coef > 1.f ? 1.f : coef;           // a NaN stays (torch.clamp keeps it)
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *norm_out = total_norm;

    const int item = blockIdx.x * kAdamWaves + wave;
    if (item >= t.num_waves) return;
    AdamScalars s;
    s.clip = h.grad_scale * coef;
    s.lerp_weight = (float)(1.0 - h.beta1);
    s.beta2 = (float)h.beta2;
    s.one_minus_beta2 = (float)(1.0 - h.beta2);
    s.eps = (float)h.eps;
    for (int ci = t.wave_first[item]; ci < t.wave_first[item + 1] && ci < t.num_chunks; ++ci) {
        const sdetr_adamw_chunk c = t.chunks[ci];
        if (!chunk_ok(t, c)) continue;
        const sdetr_adamw_record r = t.records[c.record];
        if (r.group < 0 || r.group >= h.num_groups || r.lag < 0 || r.lag >= step) continue;
        const double lr = h.groups[2 * r.group], wd = h.groups[2 * r.group + 1];
        double p1 = shared_pow[0], p2 = shared_pow[1];
        if (r.lag != 0) {         // a tensor that skipped steps (its gradient was None): its own count
            p1 = pow(h.beta1, (double)(step - r.lag));
            p2 = pow(h.beta2, (double)(step - r.lag));
        }
        s.decay = (float)(1.0 - lr * wd);
        s.neg_step_size = (float)(-(lr / (1.0 - p1)));
        s.bc2_sqrt = (float)sqrt(1.0 - p2);

        float *p = r.param + c.start;
        const float *g = r.grad + c.start;
        float *m = exp_avg + r.moment_offset + c.start;
        float *v = exp_avg_sq + r.moment_offset + c.start;
        const int head = min(c.count, to_aligned16(p));
        const bool wide = aligned16(m + head) && aligned16(v + head);
        const int body = wide ? (c.count - head) & ~3 : 0;
        const bool g_aligned = aligned16(g + head);
        if (lane < head) adamw_element(s, g[lane], p[lane], m[lane], v[lane]);
        for (int i = head + lane * 4; i < head + body; i += kWave * 4) {
            const float4 g4 = load_gradient4(g + i, g_aligned);
            float4 p4 = *reinterpret_cast<const float4 *>(p + i);
            float4 m4 = *reinterpret_cast<const float4 *>(m + i);
            float4 v4 = *reinterpret_cast<const float4 *>(v + i);
            adamw_element(s, g4.x, p4.x, m4.x, v4.x);
            adamw_element(s, g4.y, p4.y, m4.y, v4.y);
            adamw_element(s, g4.z, p4.z, m4.z, v4.z);
            adamw_element(s, g4.w, p4.w, m4.w, v4.w);
            *reinterpret_cast<float4 *>(p + i) = p4;
            *reinterpret_cast<float4 *>(m + i) = m4;
            *reinterpret_cast<float4 *>(v + i) = v4;
        }
        for (int i = head + body + lane; i < c.count; i += kWave) adamw_element(s, g[i], p[i], m[i], v[i]);
    }
}

int check_tables(const char *what, const void *records, const void *chunks, const int *wave_first, int num_records,
                 int num_chunks, int num_waves, int num_partials, const void *partials, const void *step_counter)
{
    if (num_records < 1 || num_chunks < 1 || num_waves < 1 || num_waves > num_chunks)
        return fail("%s: bad table sizes (records %d, chunks %d, wave items %d)", what, num_records, num_chunks, num_waves);
    if (num_partials < 1 || num_partials > kAdamMaxPartials || num_partials > num_waves)
        return fail("%s: num_partials = %d outside [1, min(%d, wave items = %d)]", what, num_partials, kAdamMaxPartials,
                    num_waves);
    if (!records || !chunks || !wave_first || !partials || !step_counter) return fail("%s: null pointer", what);
    return 0;
}

}  // namespace
}  // namespace sdetr

using namespace sdetr;

extern "C" int sdetr_adamw_chunk_elements(void) { return kAdamChunk; }
extern "C" int sdetr_adamw_max_partials(void) { return kAdamMaxPartials; }

extern "C" int sdetr_adamw_grad_sumsq(sdetr_stream_t stream, const sdetr_adamw_record *records, int num_records,
                                      const sdetr_adamw_chunk *chunks, int num_chunks, const int *wave_first, int num_waves,
                                      int num_partials, double *partials, int *step_counter)
{
    if (int e = check_tables("adamw_grad_sumsq", records, chunks, wave_first, num_records, num_chunks, num_waves,
                             num_partials, partials, step_counter))
        return e;
    const AdamTables t{records, chunks, wave_first, num_records, num_chunks, num_waves, num_partials};
    hipLaunchKernelGGL(adamw_sumsq_kernel, dim3((unsigned)num_partials), dim3(kBlock), 0, (hipStream_t)stream, t, partials,
                       step_counter);
    return check_launch("adamw_grad_sumsq");
}

extern "C" int sdetr_adamw_clip_step(sdetr_stream_t stream, const sdetr_adamw_record *records, int num_records,
                                     const sdetr_adamw_chunk *chunks, int num_chunks, const int *wave_first, int num_waves,
                                     int num_partials, const double *partials, const int *step_counter,
                                     const double *group_table, int num_groups, float *exp_avg, float *exp_avg_sq,
                                     double beta1, double beta2, double eps, float max_norm, float grad_scale,
                                     float *total_norm)
{
    if (int e = check_tables("adamw_clip_step", records, chunks, wave_first, num_records, num_chunks, num_waves,
                             num_partials, partials, step_counter))
        return e;
    if (!group_table || num_groups < 1) return fail("adamw_clip_step: no parameter-group table");
    if (!exp_avg || !exp_avg_sq || !total_norm) return fail("adamw_clip_step: null pointer");
    if (((uintptr_t)exp_avg & 15u) || ((uintptr_t)exp_avg_sq & 15u))
        return fail("adamw_clip_step: the moment buffers must be 16-byte aligned");
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0))
        return fail("adamw_clip_step: betas (%g, %g) must lie in [0, 1) and eps = %g must not be negative", beta1, beta2, eps);
    const AdamTables t{records, chunks, wave_first, num_records, num_chunks, num_waves, num_partials};
    const AdamHyper h{group_table, num_groups, beta1, beta2, eps, max_norm, grad_scale};
    const unsigned blocks = (unsigned)((num_waves + kAdamWaves - 1) / kAdamWaves);
    hipLaunchKernelGGL(adamw_update_kernel, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, t, h, partials, step_counter,
                       exp_avg, exp_avg_sq, total_norm);
    return check_launch("adamw_clip_step");
}

// Detection post-processing of the last decoder layer (reference models/bricks/post_process.py:PostProcess, every config's
// PostProcess(select_box_nums_for_evaluation=300)) as ONE launch: one 1024-thread workgroup per image.
//
//  1. select: the K smallest 64-bit composites (desc_bits(logit) << 32 | flat index) of the image's Nq*C entries = the K
//     largest logits, ties to the lower flat index, -0.0 == +0.0.  A radix select over the composite in up to six
//     histogram rounds in LDS (key bits 11 / 11 / 10, then the index bits 11 / 11 / 2 only while the boundary bin holds
//     more entries than are still needed -- with distinct logits the select ends after the key rounds).  Rows of at most
//     kResident = 40 960 keys are read from memory ONCE into registers (40 keys per thread); longer rows (900 x 91,
//     Objects365-sized heads) are streamed from memory (L2) in every round.
//  2. the K selected composites are appended to LDS and sorted by a bitonic sort (ascending composite = rank order).
//  3. epilogue, thread r = rank r: score = sigmoid(logit) (fp32, rounded to the logits' type), label = flat % C, box of
//     query flat / C converted (cx - 0.5w, cy - 0.5h, cx + 0.5w, cy + 0.5h) and scaled by (w, h, w, h) of the image,
//     every operation rounded on its own (no FMA contraction: torch computes them as separate kernels).
//  4. optional filters: the confidence mask (score > threshold in the score's type) and greedy class-agnostic NMS over
//     all K boxes in rank order (torchvision.ops.nms's rule).  NMS: "box j (higher rank) suppresses box i" as a
//     lower-triangular bitmask built by all waves (one IoU per lane, one ballot per 64 columns), then resolved by
//     relaxation -- a box whose suppressors are all decided is decided (kept iff none of them is kept); by induction on
//     the rank this is the sequential greedy result, and the number of rounds is the longest suppression chain.
//  5. the kept entries are compacted to the front in rank order; every slot past the count is written (score 0, label -1,
//     box 0), so no fill / memset has to run in front of the launch.
#include "common.h"
#include "topk_core.h"

#pragma clang fp contract(off)

namespace sdetr {

constexpr int kPpThreads = 1024;
constexpr int kPpWaves = kPpThreads / 64;
// keys per thread held in registers.  80 (the 900 x 91 row) spills ~62 VGPRs to scratch at the 128-VGPR budget of a
// 1024-thread workgroup; 40 fits (117 VGPRs), so rows above 40 960 keys take the streamed form
constexpr int kPpPer = 40;
constexpr int kResident = kPpPer * kPpThreads;
constexpr int kPpBatch = 16;                            // streamed form: slots loaded per thread at a time
constexpr int kPpMaxK = 1024;
constexpr int kPpRounds = 6;
constexpr int64_t kPpMaxKeys = 1 << 24;                 // the flat index lives in the composite's low 24 bits

struct PostArgs {
    const void *logits;
    int64_t logits_stride;  // elements between images
    const float *boxes;
    int64_t boxes_stride;   // floats between images
    const void *sizes;      // [B, 2] (h, w)
    int sizes_i64;
    int num_classes, n, k, kw;   // kw = 64-bit words of a K-bit row
    int use_conf, use_nms;
    float score_thr;        // in the score's type
    float iou_thr;
    void *out_scores;
    int64_t *out_labels;
    float *out_boxes;
    int *out_count;
};

// the select key of a logit: desc_bits, with the one NaN pattern whose key would be 0xffffffff moved down one place, so that
// kPpNoKey marks "no entry" unambiguously (NaN order is unspecified anyway)
constexpr uint32_t kPpNoKey = 0xffffffffu;
__device__ __forceinline__ uint32_t pp_key(float v) { return min(desc_bits(v), kPpNoKey - 1u); }

template <bool F16>
__device__ __forceinline__ float logit_at(const void *row, int i)
{
    return F16 ? act_lo((uint32_t)reinterpret_cast<const uint16_t *>(row)[i]) : reinterpret_cast<const float *>(row)[i];
}

// exclusive scan of one int per thread over the workgroup; `total` receives the sum
__device__ __forceinline__ int pp_block_scan(int v, int *wsum, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kPpWaves; ++w) {
        const int s = wsum[w];
        off += w < wave ? s : 0;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return off + x - v;
}

// LDS: [hist u32[2048] | sorted composites u64[1024]] (8 KB, aliased) and, with NMS, boxes float4[K] | areas float[K] |
// suppressor bitmask u64[K][kw]
template <bool F16, bool RESIDENT>
__global__ void __launch_bounds__(kPpThreads) detection_postprocess_kernel(PostArgs p)
{
    extern __shared__ __align__(16) unsigned char smem[];
    uint32_t *hist = reinterpret_cast<uint32_t *>(smem);
    uint64_t *cand = reinterpret_cast<uint64_t *>(smem);
    float4 *sbox = reinterpret_cast<float4 *>(smem + 8192);
    float *sarea = reinterpret_cast<float *>(smem + 8192 + (size_t)p.k * 16);
    uint64_t *sup = reinterpret_cast<uint64_t *>(smem + 8192 + (size_t)p.k * 20 + 8 - (((size_t)p.k * 20) & 7));
    __shared__ int wsum[kPpWaves];
    __shared__ int sel[3];                 // bin, entries before it, entries in it
    __shared__ int cand_n;
    __shared__ uint64_t kept_w[kPpMaxK / 64], decided_w[kPpMaxK / 64];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = p.n, K = p.k;
    const char *row = reinterpret_cast<const char *>(p.logits) + (size_t)b * p.logits_stride * (F16 ? 2 : 4);

    uint32_t kr[RESIDENT ? kPpPer : 1];
    if constexpr (RESIDENT) {
        // buffer loads: the row base in the descriptor, the whole byte offset (lane + slot) in the VGPR offset, soffset 0.
        // The range check against num_records = the row's bytes covers the VGPR and immediate offsets only -- NOT soffset
        // -- so the slot offset must not travel in soffset: slots past the row then read 0 instead of memory beyond
        // the tensor.  (No 64-bit address per load in flight either.)  The offset is laundered through an empty asm so
        // that the compiler cannot split its constant part back out into soffset.
        const __amdgpu_buffer_rsrc_t rs = make_uniform_rsrc(row, (uint32_t)n * (F16 ? 2u : 4u));
#pragma unroll
        for (int j = 0; j < kPpPer; ++j) {
            uint32_t off = (uint32_t)(j * kPpThreads + tid) * (F16 ? 2u : 4u);
            asm volatile("" : "+v"(off));
            float v;
            if constexpr (F16)
                v = act_lo((uint32_t)__builtin_amdgcn_raw_buffer_load_b16(rs, (int)off, 0, 0));
            else
                v = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)off, 0, 0));
            kr[j] = j * kPpThreads + tid < n ? pp_key(v) : kPpNoKey;
        }
    }
    // f(i, key, valid) for every key slot of this thread; whole waves call f together (ballots inside are safe).  The
    // resident slots past the row hold kPpNoKey, which no real key takes (pp_key): the histograms and the collection skip
    // it by its value (no per-slot bound test to keep live).  Counting those slots instead put every one of them into the
    // top bin of round 0 -- one LDS address, serialised atomics: a 100 x 91 row took 50 us against 35 us at 450 x 91.
    // `t` = tid laundered through an empty asm at the call: the slot indices j * 1024 + t are loop-invariant across the
    // select rounds, and hoisting all of them out of the round loop would spill the keys.
    auto visit = [&](auto &&f) {
        if constexpr (RESIDENT) {
            uint32_t t = (uint32_t)tid;
            asm volatile("" : "+v"(t));
#pragma unroll
            for (int j = 0; j < kPpPer; ++j) f(j * (uint32_t)kPpThreads + t, kr[j], true);
        } else {
            // kPpBatch loads in flight per thread before the keys are used (one at a time, every slot waited for its
            // own trip to L2: ~20 us per pass over a 900 x 91 row)
            for (int base = 0; base < n; base += kPpBatch * kPpThreads) {
                uint32_t kv[kPpBatch];
#pragma unroll
                for (int u = 0; u < kPpBatch; ++u)
                    kv[u] = pp_key(logit_at<F16>(row, min(base + u * kPpThreads + tid, n - 1)));
#pragma unroll
                for (int u = 0; u < kPpBatch; ++u) {
                    const int i = base + u * kPpThreads + tid;
                    const bool ok = i < n;
                    f((uint32_t)i, ok ? kv[u] : kPpNoKey, ok);
                }
            }
        }
    };

    // ---- 1. radix select of the K-th smallest composite (key << 32 | index), in 32-bit halves ------------------------
    // rounds 0-2: bits 31-21 / 20-10 / 9-0 of the key; rounds 3-5: bits 23-13 / 12-2 / 1-0 of the index (< 2^24)
    constexpr int kShift[kPpRounds] = {21, 10, 0, 13, 2, 0};
    constexpr int kWidth[kPpRounds] = {11, 11, 10, 11, 11, 2};
    uint32_t kpre = 0, kmask = 0, ipre = 0, imask = 0;
    int need = K, last = 0;
#pragma unroll 1
    for (int r = 0; r < kPpRounds; ++r) {
        const int sh = kShift[r];
        const uint32_t dmask = (1u << kWidth[r]) - 1u;
        const bool on_key = r < 3;
        hist[2 * tid] = 0;
        hist[2 * tid + 1] = 0;
        __syncthreads();
        if (on_key) {
            visit([&](uint32_t, uint32_t key, bool ok) {
                if (ok && key != kPpNoKey && (key & kmask) == kpre) atomicAdd(&hist[(key >> sh) & dmask], 1u);
            });
        } else {
            visit([&](uint32_t i, uint32_t key, bool ok) {
                if (ok && key == kpre && (i & imask) == ipre) atomicAdd(&hist[(i >> sh) & dmask], 1u);
            });
        }
        __syncthreads();
        const int h0 = (int)hist[2 * tid], h1 = (int)hist[2 * tid + 1];
        int total;
        const int ex = pp_block_scan(h0 + h1, wsum, total);
        if (ex < need && need <= ex + h0 + h1) {
            const bool first = need <= ex + h0;
            sel[0] = first ? 2 * tid : 2 * tid + 1;
            sel[1] = first ? ex : ex + h0;
            sel[2] = first ? h0 : h1;
        }
        __syncthreads();
        const int bin = sel[0], before = sel[1], in_bin = sel[2];
        __syncthreads();    // (sel and hist are rewritten by the next round)
        if (on_key) {
            kpre |= (uint32_t)bin << sh;
            kmask |= dmask << sh;
        } else {
            ipre |= (uint32_t)bin << sh;
            imask |= dmask << sh;
        }
        need -= before;
        last = r;
        if (in_bin == need) break;   // the whole boundary bin is taken (always true after the last round: composites are unique)
    }
    // selected: every composite whose bits down to the last round's digit are <= the prefix's -- exactly K of them
    const int lsh = kShift[last];
    auto taken = [&](uint32_t i, uint32_t key) {
        if (last < 3) return (key >> lsh) <= (kpre >> lsh);
        return key < kpre || (key == kpre && (i >> lsh) <= (ipre >> lsh));
    };

    // ---- 2. collect the K composites and sort them -----------------------------------------------------------------
    if (tid == 0) cand_n = 0;
    __syncthreads();
    visit([&](uint32_t i, uint32_t key, bool ok) {
        const bool take = ok && key != kPpNoKey && taken(i, key);
        const uint64_t bal = __ballot(take);
        if (bal) {
            int base = 0;
            if (lane == 0) base = atomicAdd(&cand_n, __popcll(bal));
            base = __shfl(base, 0, 64);
            const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
            if (take && pos < K) cand[pos] = ((uint64_t)key << 32) | i;
        }
    });
    __syncthreads();
    int P = 1;
    while (P < K) P <<= 1;
    if (tid >= K && tid < P) cand[tid] = ~0ull;
    __syncthreads();
    for (int kk = 2; kk <= P; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            const int i = tid, ixj = tid ^ j;
            if (i < P && ixj > i) {
                const uint64_t a = cand[i], c = cand[ixj];
                if ((a > c) == ((i & kk) == 0)) {
                    cand[i] = c;
                    cand[ixj] = a;
                }
            }
            __syncthreads();
        }
    }

    // ---- 3. epilogue: thread = rank ------------------------------------------------------------------------------
    const bool active = tid < K;
    float score = 0.f;
    uint32_t score_bits = 0;
    int64_t label = -1;
    float x1 = 0.f, y1 = 0.f, x2 = 0.f, y2 = 0.f;
    bool keep = false;
    if (active) {
        const uint32_t flat = (uint32_t)cand[tid] & 0xffffffu;
        const int q = (int)(flat / (uint32_t)p.num_classes);
        label = (int64_t)(flat - (uint32_t)q * (uint32_t)p.num_classes);
        const float x = logit_at<F16>(row, (int)flat);
        score = 1.f / (1.f + expf(-x));     // torch's fp32 sigmoid formula (ATen CPU / GPU: 1 / (1 + exp(-x)))
        if constexpr (F16) {
            score_bits = f32_to_act_bits(score);
            score = act_lo(score_bits);
        } else {
            score_bits = __float_as_uint(score);
        }
        const float *bx = p.boxes + (size_t)b * p.boxes_stride + (size_t)q * 4;
        const float cx = bx[0], cy = bx[1], w = bx[2], h = bx[3];
        float img_h, img_w;
        if (p.sizes_i64) {
            img_h = (float)reinterpret_cast<const int64_t *>(p.sizes)[2 * b];
            img_w = (float)reinterpret_cast<const int64_t *>(p.sizes)[2 * b + 1];
        } else {
            img_h = reinterpret_cast<const float *>(p.sizes)[2 * b];
            img_w = reinterpret_cast<const float *>(p.sizes)[2 * b + 1];
        }
        const float hw = __fmul_rn(0.5f, w), hh = __fmul_rn(0.5f, h);
        x1 = __fmul_rn(__fsub_rn(cx, hw), img_w);
        y1 = __fmul_rn(__fsub_rn(cy, hh), img_h);
        x2 = __fmul_rn(__fadd_rn(cx, hw), img_w);
        y2 = __fmul_rn(__fadd_rn(cy, hh), img_h);
        // the threshold in the score's type (torch compares `score > confidence_score` after rounding the Python float to it)
        const float thr = F16 ? act_lo(f32_to_act_bits(p.score_thr)) : p.score_thr;
        keep = p.use_conf ? score > thr : true;
    }

    // ---- 4. greedy NMS over the K boxes in rank order ----------------------------------------------------------------
    if (p.use_nms) {
        const int kw = p.kw;
        if (active) {
            sbox[tid] = make_float4(x1, y1, x2, y2);
            sarea[tid] = __fmul_rn(__fsub_rn(x2, x1), __fsub_rn(y2, y1));
        }
        if (tid < kPpMaxK / 64) {
            kept_w[tid] = 0;
            decided_w[tid] = 0;
        }
        __syncthreads();
        // sup[i][w] bit l: box j = 64 w + l < i (higher rank) overlaps box i with IoU > threshold
        for (int i = wave; i < K; i += kPpWaves) {
            const float4 bi = sbox[i];
            const float ai = sarea[i];
            for (int w = 0; w <= (i >> 6); ++w) {
                const int j = w * 64 + lane;
                bool s = false;
                if (j < i) {
                    const float4 bj = sbox[j];
                    const float iw = fmaxf(0.f, __fsub_rn(fminf(bi.z, bj.z), fmaxf(bi.x, bj.x)));
                    const float ih = fmaxf(0.f, __fsub_rn(fminf(bi.w, bj.w), fmaxf(bi.y, bj.y)));
                    const float inter = __fmul_rn(iw, ih);
                    if (inter > 0.f) s = __fdiv_rn(inter, __fsub_rn(__fadd_rn(sarea[j], ai), inter)) > p.iou_thr;
                }
                const uint64_t m = __ballot(s);
                if (lane == 0) sup[(size_t)i * kw + w] = m;
            }
        }
        __syncthreads();
        // relaxation: wave v owns the states of ranks [64 v, 64 v + 64)
        bool done = !active;
        bool kept_me = false;
        int pending = 1;
        while (pending) {
            bool now_decided = false;
            if (!done) {
                bool any_kept = false, any_open = false;
                for (int w = 0; w <= (tid >> 6); ++w) {
                    const uint64_t m = sup[(size_t)tid * kw + w];
                    any_kept |= (m & kept_w[w]) != 0;
                    any_open |= (m & ~decided_w[w]) != 0;
                }
                if (any_kept || !any_open) {
                    now_decided = true;
                    kept_me = !any_kept;
                }
            }
            const uint64_t dec = __ballot(now_decided), kep = __ballot(now_decided && kept_me);
            __syncthreads();
            if (lane == 0 && wave < kPpMaxK / 64) {
                kept_w[wave] |= kep;
                decided_w[wave] |= dec;
            }
            done = done || now_decided;
            pending = __syncthreads_or(!done);
        }
        keep = keep && kept_me;
    }

    // ---- 5. stable compaction in rank order, padding written in the kernel -------------------------------------------
    int count;
    const int pos = pp_block_scan(keep ? 1 : 0, wsum, count);
    const size_t ob = (size_t)b * K;
    auto put = [&](int slot, uint32_t sbits, int64_t lab, float a, float c, float d, float e) {
        if constexpr (F16) reinterpret_cast<uint16_t *>(p.out_scores)[ob + slot] = (uint16_t)sbits;
        else reinterpret_cast<uint32_t *>(p.out_scores)[ob + slot] = sbits;
        p.out_labels[ob + slot] = lab;
        reinterpret_cast<float4 *>(p.out_boxes)[ob + slot] = make_float4(a, c, d, e);
    };
    if (keep) put(pos, score_bits, label, x1, y1, x2, y2);
    if (tid >= count && tid < K) put(tid, 0u, -1, 0.f, 0.f, 0.f, 0.f);
    if (tid == 0) p.out_count[b] = count;
}

template <bool F16, bool RESIDENT>
static void launch(const PostArgs &a, int batch, size_t lds, hipStream_t stream)
{
    static DeviceOnce once;
    allow_dynamic_lds(detection_postprocess_kernel<F16, RESIDENT>, once, 160 * 1024 - 1024);
    hipLaunchKernelGGL((detection_postprocess_kernel<F16, RESIDENT>), dim3(batch), dim3(kPpThreads), lds, stream, a);
}

}  // namespace sdetr

using namespace sdetr;

extern "C" int sdetr_detection_postprocess(sdetr_stream_t stream, const void *logits, int logits_dtype,
                                           int64_t logits_batch_stride, const float *boxes, int64_t boxes_batch_stride,
                                           const void *target_sizes, int sizes_dtype, int batch, int num_queries,
                                           int num_classes, int k, float score_threshold, float iou_threshold,
                                           void *out_scores, int64_t *out_labels, float *out_boxes, int *out_count)
{
    if (batch < 1 || num_queries < 1 || num_classes < 1) return fail("detection_postprocess: bad sizes");
    const int64_t n = (int64_t)num_queries * num_classes;
    if (n > kPpMaxKeys) return fail("detection_postprocess: %lld entries per image exceed 2^24", (long long)n);
    if (k < 1 || k > kPpMaxK || k > n)
        return fail("detection_postprocess: k = %d outside [1, min(num_queries * num_classes, 1024)]", k);
    if (logits_dtype != SDETR_F32 && logits_dtype != kActCode)
        return fail("detection_postprocess: logits dtype %d is neither f32 nor this library's 16-bit type", logits_dtype);
    if (sizes_dtype != SDETR_F32 && sizes_dtype != SDETR_I64)
        return fail("detection_postprocess: target sizes must be f32 or int64");
    if (logits_batch_stride < n) return fail("detection_postprocess: logits batch stride smaller than num_queries * num_classes");
    if (boxes_batch_stride < (int64_t)num_queries * 4) return fail("detection_postprocess: boxes batch stride smaller than num_queries * 4");
    if (!logits || !boxes || !target_sizes || !out_scores || !out_labels || !out_boxes || !out_count)
        return fail("detection_postprocess: null pointer");
    PostArgs a{};
    a.logits = logits; a.logits_stride = logits_batch_stride; a.boxes = boxes; a.boxes_stride = boxes_batch_stride;
    a.sizes = target_sizes; a.sizes_i64 = sizes_dtype == SDETR_I64;
    a.num_classes = num_classes; a.n = (int)n; a.k = k; a.kw = (k + 63) / 64;
    a.use_conf = score_threshold > 0.f; a.use_nms = iou_threshold > 0.f;
    a.score_thr = score_threshold; a.iou_thr = iou_threshold;
    a.out_scores = out_scores; a.out_labels = out_labels; a.out_boxes = out_boxes; a.out_count = out_count;
    size_t lds = 8192;
    if (a.use_nms) lds += (size_t)k * 20 + 8 + (size_t)k * a.kw * 8;
    const bool f16 = logits_dtype != SDETR_F32, resident = n <= kResident;
    hipStream_t s = (hipStream_t)stream;
    if (f16) {
        if (resident) launch<true, true>(a, batch, lds, s);
        else launch<true, false>(a, batch, lds, s);
    } else {
        if (resident) launch<false, true>(a, batch, lds, s);
        else launch<false, false>(a, batch, lds, s);
    }
    return check_launch("detection_postprocess");
}

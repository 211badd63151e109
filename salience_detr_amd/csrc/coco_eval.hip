// COCO box evaluation (pycocotools COCOeval, iouType "bbox", default parameters) in two kernels; include/salience_hip.h
// states the record layout and the entry points, DESIGN.md the capacities.
//
// coco_update_kernel: one workgroup per image of the batch.
//  (0) every workgroup counts, image by image, the detection rows (sum over categories of min(100, detections)) and the
//      ground-truth rows (categories with ground truths) of ALL images of the batch: LDS histograms over the category
//      index.  The rows before its own image are its append position, the sum is the batch total: a prefix, no global
//      atomics, the same bytes on every run.  Its own image comes last, so its histograms stay in LDS.
//  (1) rank of every detection within its (image, category): score descending, ties to the earlier detection; the two
//      histograms become offsets (exclusive scans), `dorder` / `gorder` list the image's detections and ground truths
//      category by category, detections in rank order.
//  (2) a wave per category present (categories wave, wave + 4, ..).  The category's ground truths go to the wave's LDS
//      (box, ignore bit per area range, crowd bit) and are ordered non-ignored first per area range (ballot compaction).
//      Lane a * 10 + t owns the greedy walk of area range a at threshold t (40 of 64 lanes): its matched-ground-truth
//      set is a 128-bit register mask.  Per detection, in rank order, the 64 lanes compute the float64 IoU row into
//      LDS, the 40 lanes walk it, and two ballots ARE the detection's matched / ignored words.
//
// coco_accumulate_kernel: one workgroup per (category, area range, maxDet) over the category's records in final order.
//  pass 1: totals of tp = matched & ~ignored and fp = ~matched & ~ignored per threshold over the records with
//          rank < maxDet;
//  pass 2: chunks of kChunk records from the LAST to the first.  tp_i = total - (tp strictly after i), so the carried
//          state runs the same way as the right-to-left running maximum of the precision: per threshold one integer
//          scan (tp | fp << 32) and one float64 max scan per chunk, carries in LDS.  Recall threshold r is answered by
//          exactly one record, the first with rc_i >= thr_r, i.e. rc_(i-1) < thr_r <= rc_i: that record's thread writes
//          the running maximum and its score into the LDS answer table (no two writers for one slot).  thr_r <= 0 is
//          answered by the first record: the maximum over everything, and its score.
#include "common.h"

#pragma clang fp contract(off)

namespace sdetr {
namespace {

constexpr int kT = SDETR_COCO_THRESHOLDS;
constexpr int kR = SDETR_COCO_RECALL_POINTS;
constexpr int kA = SDETR_COCO_AREAS;
constexpr int kMaxDets = SDETR_COCO_MAX_DETS;
constexpr int kDetWords = SDETR_COCO_DET_WORDS;
constexpr int kGtWords = SDETR_COCO_GT_WORDS;
constexpr int kMaxCat = SDETR_COCO_MAX_CATEGORIES;
constexpr int kMaxDetImg = SDETR_COCO_MAX_DET_PER_IMAGE;
constexpr int kMaxGtImg = SDETR_COCO_MAX_GT_PER_IMAGE;
constexpr int kGtCap = SDETR_COCO_GT_CAP;
constexpr int kChunk = SDETR_COCO_ACC_CHUNK;
constexpr int kWaves = kBlock / kWave;
constexpr int kPer = kChunk / kBlock;          // records of a chunk per thread
static_assert(kGtWords == 3 + kA && kDetWords == 5, "record layouts");
static_assert(kA * kT <= kWave, "one lane per (area range, threshold)");
static_assert(kGtCap == 2 * kWave, "the matched set is two 64-bit masks, the IoU row two rounds of the wave");
static_assert(kChunk % kBlock == 0, "a chunk is a whole number of records per thread");

__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// sum over the workgroup (integers: any order gives the same bits); every thread returns it
__device__ __forceinline__ long long block_sum_i64(long long x, long long *tmp)
{
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0) tmp[threadIdx.x / kWave] = x;
    __syncthreads();
    long long s = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += tmp[w];
    __syncthreads();
    return s;
}

// a[0 .. n) -> its exclusive prefix in place, a[n] = the total (n <= kMaxCat; a[] complete before the call)
__device__ void block_exclusive_scan(int *a, int n, long long *tmp)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int per = (n + kBlock - 1) / kBlock;
    const int lo = min(n, (int)threadIdx.x * per), hi = min(n, lo + per);
    int own = 0;
    for (int i = lo; i < hi; ++i) own += a[i];
    int inc = own;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int y = __shfl_up(inc, o, kWave);
        if (lane >= o) inc += y;
    }
    if (lane == kWave - 1) tmp[wave] = inc;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        if (w < wave) before += (int)tmp[w];
        total += (int)tmp[w];
    }
    int run = before + inc - own;
    for (int i = lo; i < hi; ++i) {
        const int v = a[i];
        a[i] = run;
        run += v;
    }
    if (threadIdx.x == 0) a[n] = total;
    __syncthreads();
}

struct CocoUpdate {
    const float *scores;
    const int64_t *labels;
    const float *boxes;
    const int *count;
    int batch, k;
    const float *gt_boxes;
    const int64_t *gt_labels;
    const double *gt_area;
    const uint8_t *gt_crowd;
    const int *gt_count;
    const int64_t *image_ids;
    int max_gt;
    const int *lut;
    int lut_size, num_cat;
    const double *thr;
    int64_t *det;
    int64_t *gt;
    int *totals;
};

__device__ __forceinline__ int category_of(const CocoUpdate &p, int64_t label)
{
    if (label < 0 || label >= (int64_t)p.lut_size) return -1;
    const int c = p.lut[label];
    return (c >= 0 && c < p.num_cat) ? c : -1;
}

__device__ __forceinline__ double area_lo(int a) { return a == 2 ? 1024.0 : a == 3 ? 9216.0 : 0.0; }
__device__ __forceinline__ double area_hi(int a) { return a == 1 ? 1024.0 : a == 2 ? 9216.0 : 1e10; }

__global__ void __launch_bounds__(kBlock) coco_update_kernel(CocoUpdate p)
{
    __shared__ int dh[kMaxCat + 1], gh[kMaxCat + 1], pg[kMaxCat + 1];
    __shared__ short dcat[kMaxDetImg], drank[kMaxDetImg], dorder[kMaxDetImg], gcat[kMaxGtImg], gorder[kMaxGtImg];
    __shared__ float dscore[kMaxDetImg];
    __shared__ long long tmp[kWaves];
    __shared__ float4 wbox[kWaves][kGtCap];
    __shared__ double wrow[kWaves][kGtCap];
    __shared__ unsigned char wflag[kWaves][kGtCap];          // bit a: ignored in area range a; bit 4: crowd
    __shared__ unsigned char wperm[kWaves][kA][kGtCap];      // ground truths of the category, non-ignored first

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int b = blockIdx.x, K = p.num_cat, B = p.batch, k = p.k, G = p.max_gt;

    // ---- (0) rows of every image of the batch; the own image last
    int det_before = 0, det_total = 0, gt_before = 0, gt_total = 0, nd = 0, ng = 0;
    for (int it = 0; it < B; ++it) {
        const int img = (b + 1 + it) % B;
        const bool own = img == b;
        for (int c = tid; c <= K; c += kBlock) {
            dh[c] = 0;
            gh[c] = 0;
        }
        __syncthreads();
        nd = min(max(p.count[img], 0), k);
        ng = min(max(p.gt_count[img], 0), G);
        for (int j = tid; j < nd; j += kBlock) {
            const int c = category_of(p, p.labels[(size_t)img * k + j]);
            if (own) {
                dcat[j] = (short)c;
                dscore[j] = p.scores[(size_t)img * k + j];
            }
            if (c >= 0) atomicAdd(&dh[c], 1);
        }
        for (int g = tid; g < ng; g += kBlock) {
            const int c = category_of(p, p.gt_labels[(size_t)img * G + g]);
            if (own) gcat[g] = (short)c;
            if (c >= 0) atomicAdd(&gh[c], 1);
        }
        __syncthreads();
        long long part = 0;
        for (int c = tid; c < K; c += kBlock) part += (long long)min(dh[c], kMaxDets) + ((long long)(gh[c] > 0) << 32);
        const long long s = block_sum_i64(part, tmp);
        const int rows_d = (int)(s & 0xffffffffll), rows_g = (int)(s >> 32);
        det_total += rows_d;
        gt_total += rows_g;
        if (img < b) {
            det_before += rows_d;
            gt_before += rows_g;
        }
    }

    // ---- (1) ranks, offsets, orders
    for (int j = tid; j < nd; j += kBlock) {
        const int c = dcat[j];
        int r = 0;
        if (c >= 0) {
            const float s = dscore[j];
            for (int i = 0; i < nd; ++i) r += (dcat[i] == c && (dscore[i] > s || (dscore[i] == s && i < j))) ? 1 : 0;
        }
        drank[j] = (short)min(r, kMaxDetImg);
    }
    for (int c = tid; c < K; c += kBlock) {
        dh[c] = min(dh[c], kMaxDets);
        pg[c] = gh[c] > 0 ? 1 : 0;
    }
    __syncthreads();
    block_exclusive_scan(dh, K, tmp);
    block_exclusive_scan(gh, K, tmp);
    block_exclusive_scan(pg, K, tmp);
    for (int j = tid; j < nd; j += kBlock) {
        const int c = dcat[j];
        if (c >= 0 && drank[j] < kMaxDets) dorder[dh[c] + drank[j]] = (short)j;
    }
    for (int g = tid; g < ng; g += kBlock) {
        const int c = gcat[g];
        if (c < 0) continue;
        int at = 0;
        for (int i = 0; i < g; ++i) at += gcat[i] == c ? 1 : 0;
        gorder[gh[c] + at] = (short)g;
    }
    __syncthreads();

    // ---- (2) a wave per category
    const int64_t image_id = p.image_ids[b];
    const bool active = lane < kA * kT;
    const int a = active ? lane / kT : 0, t = lane % kT;
    const double thr0 = fmin(p.thr[t], 1.0 - 1e-10);
    const double lo = area_lo(a), hi = area_hi(a);
    for (int c = wave; c < K; c += kWaves) {
        const int cd = dh[c + 1] - dh[c], cg_all = gh[c + 1] - gh[c];
        if (cd == 0 && cg_all == 0) continue;
        const int cg = min(cg_all, kGtCap);
        for (int i = lane; i < cg; i += kWave) {
            const size_t g = (size_t)b * G + gorder[gh[c] + i];
            const float4 box = *reinterpret_cast<const float4 *>(p.gt_boxes + g * 4);
            const double ar = p.gt_area[g];
            const bool crowd = p.gt_crowd[g] != 0;
            unsigned f = crowd ? 16u : 0u;
#pragma unroll
            for (int q = 0; q < kA; ++q) f |= (crowd || ar < area_lo(q) || ar > area_hi(q)) ? (1u << q) : 0u;
            wbox[wave][i] = box;
            wflag[wave][i] = (unsigned char)f;
        }
        wave_sync();
        long long npig[kA];
        const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
        for (int q = 0; q < kA; ++q) {
            const int i0 = lane, i1 = lane + kWave;
            const bool v0 = i0 < cg, v1 = i1 < cg;
            const bool n0 = v0 && !((wflag[wave][v0 ? i0 : 0] >> q) & 1), n1 = v1 && !((wflag[wave][v1 ? i1 : 0] >> q) & 1);
            const unsigned long long bn0 = __ballot(n0), bn1 = __ballot(n1), bi0 = __ballot(v0 && !n0), bi1 = __ballot(v1 && !n1);
            const int c0 = __popcll(bn0), nn = c0 + __popcll(bn1), ig0 = __popcll(bi0);
            if (v0) wperm[wave][q][n0 ? __popcll(bn0 & below) : nn + __popcll(bi0 & below)] = (unsigned char)i0;
            if (v1) wperm[wave][q][n1 ? c0 + __popcll(bn1 & below) : nn + ig0 + __popcll(bi1 & below)] = (unsigned char)i1;
            npig[q] = cg_all > kGtCap ? -1 : nn;      // over capacity: the evaluator raises on this record
        }
        wave_sync();
        if (cg_all > 0 && lane < kGtWords) {
            int64_t w = lane == 0 ? image_id : (int64_t)c;
#pragma unroll
            for (int q = 0; q < kA; ++q) w = lane == 2 + q ? npig[q] : w;
            w = lane == 2 + kA ? (int64_t)cg_all : w;
            p.gt[((size_t)gt_before + pg[c]) * kGtWords + lane] = w;
        }

        unsigned long long mlo = 0, mhi = 0;       // ground truths (positions in wbox) this lane has matched
        for (int d = 0; d < cd; ++d) {
            const int j = dorder[dh[c] + d];
            const float4 bx = *reinterpret_cast<const float4 *>(p.boxes + ((size_t)b * k + j) * 4);
            const double dx1 = bx.x, dy1 = bx.y, dx2 = bx.z, dy2 = bx.w;
            const double darea = (dx2 - dx1) * (dy2 - dy1);
            for (int i = lane; i < cg; i += kWave) {
                const float4 gb = wbox[wave][i];
                const double gx1 = gb.x, gy1 = gb.y, gx2 = gb.z, gy2 = gb.w;
                const double iw = fmin(dx2, gx2) - fmax(dx1, gx1), ih = fmin(dy2, gy2) - fmax(dy1, gy1);
                double iou = 0.0;
                if (iw > 0.0 && ih > 0.0) {
                    const double inter = iw * ih;
                    const double uni = (wflag[wave][i] & 16u) ? darea : darea + (gx2 - gx1) * (gy2 - gy1) - inter;
                    iou = inter / uni;
                }
                wrow[wave][i] = iou;
            }
            wave_sync();
            int m = -1;
            bool m_ign = false;
            if (active) {
                double best = thr0;
                for (int i = 0; i < cg; ++i) {
                    const int g = wperm[wave][a][i];
                    const unsigned f = wflag[wave][g];
                    const bool g_ign = (f >> a) & 1u;
                    const bool taken = g < kWave ? (mlo >> g) & 1ull : (mhi >> (g - kWave)) & 1ull;
                    if (taken && !(f & 16u)) continue;
                    if (m >= 0 && !m_ign && g_ign) break;
                    const double v = wrow[wave][g];
                    if (v < best) continue;
                    best = v;
                    m = g;
                    m_ign = g_ign;
                }
                if (m >= 0) {
                    if (m < kWave) mlo |= 1ull << m;
                    else mhi |= 1ull << (m - kWave);
                }
            }
            const bool matched = active && m >= 0;
            const bool ignored = active && (matched ? m_ign : (darea < lo || darea > hi));
            const unsigned long long bm = __ballot(matched), bi = __ballot(ignored);
            if (lane < kDetWords) {
                const double sc = (double)dscore[j];
                int64_t w = image_id;
                w = lane == 1 ? ((int64_t)c | ((int64_t)d << 32)) : w;
                w = lane == 2 ? (int64_t)__double_as_longlong(sc) : w;
                w = lane == 3 ? (int64_t)bm : w;
                w = lane == 4 ? (int64_t)bi : w;
                p.det[((size_t)det_before + dh[c] + d) * kDetWords + lane] = w;
            }
            wave_sync();
        }
    }

    // ---- padding rows behind the batch's real rows, split over the workgroups; the totals
    for (int64_t s = (int64_t)det_total + b + (int64_t)B * tid; s < (int64_t)B * k; s += (int64_t)B * kBlock) {
        p.det[s * kDetWords + 0] = -1;
        p.det[s * kDetWords + 1] = -1;
        p.det[s * kDetWords + 2] = 0;
        p.det[s * kDetWords + 3] = 0;
        p.det[s * kDetWords + 4] = 0;
    }
    for (int64_t s = (int64_t)gt_total + b + (int64_t)B * tid; s < (int64_t)B * G; s += (int64_t)B * kBlock) {
        p.gt[s * kGtWords + 0] = -1;
        p.gt[s * kGtWords + 1] = -1;
#pragma unroll
        for (int q = 0; q <= kA; ++q) p.gt[s * kGtWords + 2 + q] = 0;
    }
    if (b == 0 && tid == 0) {
        p.totals[0] = det_total;
        p.totals[1] = gt_total;
    }
}

struct CocoAccumulate {
    const int64_t *rec;
    int64_t n;
    const int64_t *first;
    const int64_t *npig;
    int num_cat;
    const double *rthr;
    double *precision, *recall, *scores;
};

__global__ void __launch_bounds__(kBlock) coco_accumulate_kernel(CocoAccumulate p)
{
    __shared__ double ans_p[kT][kR], ans_s[kT][kR];
    __shared__ double rthr[kR];
    __shared__ unsigned cbits[kChunk];          // bit t: matched at t; bit 16 + t: ignored at t; bit 31: rank < maxDet
    __shared__ double cscore[kChunk];
    __shared__ long long tmp[kWaves];
    __shared__ double tmpd[kWaves];
    __shared__ long long s_tot[kT], s_after[kT];   // tp | fp << 32: over the category; over the chunks already done
    __shared__ double s_max[kT];                   // running maximum of the precision over the chunks already done

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int K = p.num_cat;
    const int m = blockIdx.x % 3, a = (blockIdx.x / 3) % kA, c = blockIdx.x / (3 * kA);
    const int max_det = m == 0 ? 1 : m == 1 ? 10 : kMaxDets;
    const int64_t begin = min(max(p.first[c], (int64_t)0), p.n), end = min(max(p.first[c + 1], begin), p.n);
    const long long npig = p.npig[c * kA + a];
    const double eps = 2.220446049250313e-16;      // np.spacing(1)
    const size_t recall_at = ((size_t)c * kA + a) * 3 + m;            // + t * K * 12
    const size_t stride_t = (size_t)K * kA * 3;

    if (npig <= 0) {
        for (int i = tid; i < kT * kR; i += kBlock) {
            p.precision[(size_t)i * stride_t + recall_at] = -1.0;
            p.scores[(size_t)i * stride_t + recall_at] = -1.0;
        }
        if (tid < kT) p.recall[(size_t)tid * stride_t + recall_at] = -1.0;
        return;
    }
    for (int i = tid; i < kT * kR; i += kBlock) {
        (&ans_p[0][0])[i] = 0.0;
        (&ans_s[0][0])[i] = 0.0;
    }
    if (tid < kR) rthr[tid] = p.rthr[tid];

    // ---- pass 1: totals, and the first record with rank < maxDet
    long long tot[kT];
#pragma unroll
    for (int t = 0; t < kT; ++t) tot[t] = 0;
    long long first_kept = end;
    for (int64_t i = begin + tid; i < end; i += kBlock) {
        const int64_t *r = p.rec + i * kDetWords;
        if ((int)(r[1] >> 32) >= max_det) continue;
        first_kept = min(first_kept, (long long)i);
        const unsigned mt = (unsigned)((uint64_t)r[3] >> (a * kT)), ig = (unsigned)((uint64_t)r[4] >> (a * kT));
#pragma unroll
        for (int t = 0; t < kT; ++t) {
            const long long is_tp = (mt >> t) & ~(ig >> t) & 1u, is_fp = ~(mt >> t) & ~(ig >> t) & 1u;
            tot[t] += is_tp | (is_fp << 32);
        }
    }
#pragma unroll
    for (int t = 0; t < kT; ++t) {
        const long long s = block_sum_i64(tot[t], tmp);
        if (tid == 0) {
            s_tot[t] = s;
            s_after[t] = 0;
            s_max[t] = -1.0;
        }
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) first_kept = min(first_kept, (long long)__shfl_xor(first_kept, o, kWave));
    if (lane == 0) tmp[wave] = first_kept;
    __syncthreads();
    first_kept = min(min(tmp[0], tmp[1]), min(tmp[2], tmp[3]));
    __syncthreads();

    // ---- pass 2: chunks from the last to the first
    const int64_t chunks = (end - begin + kChunk - 1) / kChunk;
    for (int64_t ch = chunks - 1; ch >= 0; --ch) {
        const int64_t base = begin + ch * kChunk;
        const int cnt = (int)min((int64_t)kChunk, end - base);
        for (int i = tid; i < kChunk; i += kBlock) {
            unsigned bits = 0;
            double sc = 0.0;
            if (i < cnt) {
                const int64_t *r = p.rec + (base + i) * kDetWords;
                if ((int)(r[1] >> 32) < max_det) {
                    bits = 0x80000000u | ((unsigned)((uint64_t)r[3] >> (a * kT)) & 0x3ffu) |
                           (((unsigned)((uint64_t)r[4] >> (a * kT)) & 0x3ffu) << 16);
                    sc = __longlong_as_double(r[2]);
                }
            }
            cbits[i] = bits;
            cscore[i] = sc;
        }
        __syncthreads();
        for (int t = 0; t < kT; ++t) {
            const long long total = s_tot[t], done = s_after[t];
            const double done_max = s_max[t];
            // the thread's kPer consecutive records
            long long f[kPer], own = 0;
#pragma unroll
            for (int q = 0; q < kPer; ++q) {
                const unsigned bits = cbits[tid * kPer + q];
                const long long kept = bits >> 31, mt = (bits >> t) & 1u, ig = (bits >> (16 + t)) & 1u;
                f[q] = (kept & mt & ~ig & 1) | ((kept & ~mt & ~ig & 1) << 32);
                own += f[q];
            }
            long long inc = own;                 // sum over lanes >= lane
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {
                const long long y = __shfl_down(inc, o, kWave);
                if (lane + o < kWave) inc += y;
            }
            if (lane == 0) tmp[wave] = inc;
            __syncthreads();
            long long after = done + inc - own, chunk_total = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                if (w > wave) after += tmp[w];
                chunk_total += tmp[w];
            }
            // inclusive counts at each record, its precision, the running maximum inside the thread
            long long tp[kPer];
            double pr[kPer], own_max = -1.0;
#pragma unroll
            for (int q = kPer - 1; q >= 0; --q) {
                const long long at = total - after;          // tp | fp << 32, inclusive of this record
                tp[q] = at & 0xffffffffll;
                const long long fp = at >> 32;
                const bool kept = cbits[tid * kPer + q] >> 31;
                const double v = kept ? (double)tp[q] / ((double)(fp + tp[q]) + eps) : -1.0;
                own_max = fmax(own_max, v);
                pr[q] = own_max;
                after += f[q];
            }
            double inc_max = own_max;            // maximum over lanes >= lane
#pragma unroll
            for (int o = 1; o < kWave; o <<= 1) {
                const double y = __shfl_down(inc_max, o, kWave);
                if (lane + o < kWave) inc_max = fmax(inc_max, y);
            }
            // (the maximum over the lanes ABOVE this one: shift by one lane)
            double above = __shfl_down(inc_max, 1, kWave);
            if (lane == kWave - 1) above = -1.0;
            if (lane == 0) tmpd[wave] = inc_max;
            __syncthreads();
            double chunk_max = -1.0;
            above = fmax(above, done_max);
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
                if (w > wave) above = fmax(above, tmpd[w]);
                chunk_max = fmax(chunk_max, tmpd[w]);
            }
#pragma unroll
            for (int q = 0; q < kPer; ++q) {
                if (!(f[q] & 1)) continue;               // only a true positive moves the recall
                const double rc = (double)tp[q] / (double)npig, rc_prev = (double)(tp[q] - 1) / (double)npig;
                int lo = 0, hi = kR;                      // first r with rthr[r] > rc_prev
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (rthr[mid] > rc_prev) hi = mid;
                    else lo = mid + 1;
                }
                const double value = fmax(pr[q], above);
                for (int r = lo; r < kR && rthr[r] <= rc; ++r) {
                    if (rthr[r] <= 0.0) continue;         // answered by the first record, below
                    ans_p[t][r] = value;
                    ans_s[t][r] = cscore[tid * kPer + q];
                }
            }
            __syncthreads();
            if (tid == 0) {
                s_after[t] = done + chunk_total;
                s_max[t] = fmax(done_max, chunk_max);
            }
        }
        __syncthreads();
    }

    // ---- recall thresholds <= 0: the first record; the recall; the answers
    if (first_kept < end) {
        const double sc = __longlong_as_double(p.rec[first_kept * kDetWords + 2]);
        for (int i = tid; i < kT * kR; i += kBlock) {
            const int t = i / kR, r = i % kR;
            if (rthr[r] <= 0.0) {
                ans_p[t][r] = s_max[t];
                ans_s[t][r] = sc;
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < kT * kR; i += kBlock) {
        p.precision[(size_t)i * stride_t + recall_at] = (&ans_p[0][0])[i];
        p.scores[(size_t)i * stride_t + recall_at] = (&ans_s[0][0])[i];
    }
    if (tid < kT) p.recall[(size_t)tid * stride_t + recall_at] = (double)(s_tot[tid] & 0xffffffffll) / (double)npig;
}

}  // namespace
}  // namespace sdetr

using namespace sdetr;

extern "C" int sdetr_coco_eval_gt_capacity(void) { return kGtCap; }
extern "C" int sdetr_coco_eval_chunk_records(void) { return kChunk; }

extern "C" int sdetr_coco_eval_update(sdetr_stream_t stream, const float *scores, const int64_t *labels, const float *boxes,
                                      const int *count, int batch, int k, const float *gt_boxes, const int64_t *gt_labels,
                                      const double *gt_area, const uint8_t *gt_crowd, const int *gt_count,
                                      const int64_t *image_ids, int max_gt, const int *category_lut, int lut_size,
                                      int num_categories, const double *iou_thresholds, int64_t *det_records,
                                      int64_t *gt_records, int *totals)
{
    if (batch < 0 || k < 1 || k > kMaxDetImg)
        return fail("coco_eval_update: bad dims (batch %d, k %d; k in [1, %d])", batch, k, kMaxDetImg);
    if (max_gt < 1 || max_gt > kMaxGtImg)
        return fail("coco_eval_update: max_gt = %d outside [1, %d]", max_gt, kMaxGtImg);
    if (num_categories < 1 || num_categories > kMaxCat || lut_size < 1)
        return fail("coco_eval_update: %d categories (at most %d), table of %d", num_categories, kMaxCat, lut_size);
    if (batch == 0) return 0;
    if (!scores || !labels || !boxes || !count || !gt_boxes || !gt_labels || !gt_area || !gt_crowd || !gt_count ||
        !image_ids || !category_lut || !iou_thresholds || !det_records || !gt_records || !totals)
        return fail("coco_eval_update: null pointer");
    if (((uintptr_t)boxes & 15u) || ((uintptr_t)gt_boxes & 15u))
        return fail("coco_eval_update: the box tensors must be 16-byte aligned");
    const CocoUpdate p{scores, labels, boxes, count, batch, k, gt_boxes, gt_labels, gt_area, gt_crowd, gt_count, image_ids,
                       max_gt, category_lut, lut_size, num_categories, iou_thresholds, det_records, gt_records, totals};
    hipLaunchKernelGGL(coco_update_kernel, dim3((unsigned)batch), dim3(kBlock), 0, (hipStream_t)stream, p);
    return check_launch("coco_eval_update");
}

extern "C" int sdetr_coco_eval_accumulate(sdetr_stream_t stream, const int64_t *records, int64_t num_records,
                                          const int64_t *category_first, const int64_t *npig, int num_categories,
                                          const double *recall_thresholds, double *precision, double *recall,
                                          double *scores)
{
    if (num_records < 0 || num_categories < 1 || num_categories > kMaxCat)
        return fail("coco_eval_accumulate: bad dims (%lld records, %d categories; at most %d)", (long long)num_records,
                    num_categories, kMaxCat);
    if ((num_records > 0 && !records) || !category_first || !npig || !recall_thresholds || !precision || !recall || !scores)
        return fail("coco_eval_accumulate: null pointer");
    const CocoAccumulate p{records, num_records, category_first, npig, num_categories, recall_thresholds, precision, recall,
                           scores};
    hipLaunchKernelGGL(coco_accumulate_kernel, dim3((unsigned)(num_categories * kA * 3)), dim3(kBlock), 0,
                       (hipStream_t)stream, p);
    return check_launch("coco_eval_accumulate");
}

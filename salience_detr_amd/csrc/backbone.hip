// The detector's backbone (row N0): eval-mode ResNet with FrozenBatchNorm2d (reference models/backbones/resnet.py,
// models/bricks/misc.py:9-57) and the image batching in front of it (base_detector.py:114-126, util/misc.py:75-104).
//
//   backbone_pack_kernel      folds FrozenBatchNorm2d into the conv (w' = w * g / sqrt(var + eps), b' = beta - mean * g /
//                             sqrt(var + eps)) and writes w' in the GEMM's reduction order: three bf16 planes of the exact
//                             truncating split (fp32 mode) or one 16-bit plane rounded to nearest (16-bit mode)
//   backbone_conv_kernel      implicit-GEMM convolution C[pixel, co] = sum_k X[pixel, k] W'[co, k] on the matrix cores,
//                             epilogue relu?(acc + b'[co] (+ residual)), channels-last output in the compute dtype and,
//                             for the last block of a returned stage, an fp32 NCHW copy; split over K when the tile grid
//                             is small, the pieces summed in a fixed order by backbone_splitk_kernel (no atomics)
//                             The same kernel with another A-tile loader (backbone_conv_core.h) is the modulated
//                             deformable 3x3 product of a DCN stage (op 2: four masked bilinear corners per tap summed
//                             into the tile, fp32 or rounded once to 16 bits) and the exact product on 16-bit
//                             activations in front of it (op 3: the offsets and mask logits, fp32 out at any precision)
//   backbone_maxpool_kernel   3x3 stride-2 pad-1 max pool, channels-last
//   backbone_batch_kernel     normalise (ImageNet mean / std) and pad a list of images into one canvas + padding mask
//
// Tiles: 256 pixels x 128 output channels x 32 reduction indices, 8 waves of 64 x 64 (2 x 2 v_mfma_f32_32x32x16 per
// 16-deep half step), the shape of gemm_x3.hip's second-generation kernel: the activation operand A (pixels) in LDS as
// fp32 rows split into three bf16 terms fragment by fragment (fp32 mode) or as 16-bit rows; the weight operand B as its
// pre-split planes.  Two LDS stages: the next tile is loaded into registers while the current one is multiplied, one
// barrier per step.  Activations between layers are channels-last [B, H, W, C] in the compute dtype (fp32 or the
// library's 16-bit type), so with C a multiple of 32 one reduction tile is one filter tap of 32 contiguous channels
// (reduction order k = (ky * kw + kx) * C + c).  The stem reads the fp32 NCHW canvas directly with a per-element gather
// (reduction order k = c * kh * kw + ky * kw + kx, K = 147 padded to 160 with zero weight columns).
#include <algorithm>
#include <type_traits>

#include "backbone_conv_core.h"
#include "common.h"
#include "image_norm.h"
#include "plan.h"

namespace sdetr {
namespace {

// w' and b' of FrozenBatchNorm2d folded into the conv; planes [pl][co][kpad], zero past K
__global__ void __launch_bounds__(256) backbone_pack_kernel(const float *w, const float *gamma, const float *beta,
                                                            const float *mean, const float *var, float eps, int co, int ci,
                                                            int ks, int kpad, int layout, int precision, uint16_t *out,
                                                            float *bias)
{
    const int kk2 = ks * ks, K = ci * kk2;
    const int64_t total = (int64_t)co * kpad, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int o = (int)(e / kpad), k = (int)(e - (int64_t)o * kpad);
        const float s = gamma[o] / sqrtf(var[o] + eps);
        float v = 0.f;
        if (k < K) {
            int64_t src;
            if (layout == 0) {   // k = tap * ci + c
                const int tap = k / ci, cc = k - tap * ci;
                src = ((int64_t)o * ci + cc) * kk2 + tap;
            } else {
                src = (int64_t)o * K + k;
            }
            v = w[src] * s;
        }
        if (k == 0) bias[o] = beta[o] - mean[o] * s;
        if (precision == 0) {
            const float r1 = v - __uint_as_float(__float_as_uint(v) & 0xffff0000u);
            const float r2 = r1 - __uint_as_float(__float_as_uint(r1) & 0xffff0000u);
            out[e] = (uint16_t)(__float_as_uint(v) >> 16);
            out[total + e] = (uint16_t)(__float_as_uint(r1) >> 16);
            out[2 * total + e] = (uint16_t)(__float_as_uint(r2) >> 16);
        } else {
            out[e] = (uint16_t)f32_to_act_bits(v);
        }
    }
}

// 16 bytes (4 fp32 | 8 16-bit channels) of one output pixel per thread; padding taps never win (PyTorch's -inf)
template <bool X3>
__global__ void __launch_bounds__(256) backbone_maxpool_kernel(const char *x, int batch, int h, int w, int c, int ho, int wo,
                                                               char *out)
{
    constexpr int per = X3 ? 4 : 8;
    const int vec = c / per;
    const int64_t total = (int64_t)batch * ho * wo * vec, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int v = (int)(e % vec);
        const int64_t pix = e / vec;
        const int ox = (int)(pix % wo), oy = (int)((pix / wo) % ho), n = (int)(pix / ((int64_t)wo * ho));
        float mx[per];
#pragma unroll
        for (int i = 0; i < per; ++i) mx[i] = -INFINITY;
        for (int dy = 0; dy < 3; ++dy) {
            const int iy = 2 * oy - 1 + dy;
            if (iy < 0 || iy >= h) continue;
            for (int dx = 0; dx < 3; ++dx) {
                const int ix = 2 * ox - 1 + dx;
                if (ix < 0 || ix >= w) continue;
                const uint4 q = *reinterpret_cast<const uint4 *>(x + ((((int64_t)n * h + iy) * w + ix) * c + v * per) *
                                                                         (X3 ? 4 : 2));
                const uint32_t u[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (X3) {
                        mx[i] = fmaxf(mx[i], __uint_as_float(u[i]));
                    } else {
                        mx[2 * i] = fmaxf(mx[2 * i], act_lo(u[i]));
                        mx[2 * i + 1] = fmaxf(mx[2 * i + 1], act_hi(u[i]));
                    }
                }
            }
        }
        uint4 r;
        if (X3) r = make_uint4(__float_as_uint(mx[0]), __float_as_uint(mx[1]), __float_as_uint(mx[2]), __float_as_uint(mx[3]));
        else r = make_uint4(pack_act2(mx[0], mx[1]), pack_act2(mx[2], mx[3]), pack_act2(mx[4], mx[5]), pack_act2(mx[6], mx[7]));
        *reinterpret_cast<uint4 *>(out + e * 16) = r;
    }
}

struct BatchArgs {
    const void *img[kBMaxImages];
    int h[kBMaxImages], w[kBMaxImages];
    int batch, hp, wp, is_u8, normalize;
    float *canvas;
    uint8_t *mask;
};

// canvas[b, ch, y, x] = (v - mean[ch]) / std[ch] inside image b (v = u8 / 255 for uint8 input), 0 on padding; without
// `normalize` the value itself (bit for bit)
__global__ void __launch_bounds__(256) backbone_batch_kernel(BatchArgs a)
{
    const int64_t plane = (int64_t)a.hp * a.wp, total = a.batch * plane, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        const int b = (int)(e / plane);
        const int64_t p = e - b * plane;
        const int y = (int)(p / a.wp), x = (int)(p - (int64_t)y * a.wp);
        const int h = a.h[b], w = a.w[b];
        const bool in = y < h && x < w;
        for (int ch = 0; ch < 3; ++ch) {
            float v = 0.f;
            if (in) {
                const int64_t src = ((int64_t)ch * h + y) * w + x;
                const float raw = a.is_u8 ? image_unit_from_u8((float)reinterpret_cast<const uint8_t *>(a.img[b])[src])
                                          : reinterpret_cast<const float *>(a.img[b])[src];
                v = a.normalize ? image_normalize(raw, ch) : raw;
            }
            a.canvas[((int64_t)b * 3 + ch) * plane + p] = v;
        }
        a.mask[e] = in ? 0 : 1;
    }
}

// ------------------------------------------------------------------------------------------------------------ host

// validated kernel arguments of one conv op (precision 0 fp32, 1 the library's 16-bit type).  Kinds: 0 the conv; 2 the
// deformable product (kernel 3, padding 1, the reduction never split); 3 the exact conv (three-plane weight and fp32 output
// at either precision, no residual).
int make_conv(const sdetr_backbone_op &o, int precision, BConv &c)
{
    const char *what = o.op == 2 ? "sdetr_backbone (deformable conv)" : o.op == 3 ? "sdetr_backbone (exact conv)"
                                                                                  : "sdetr_backbone (conv)";
    if (precision != 0 && precision != 1) return fail("%s: precision must be 0 or 1", what);
    if (!o.x || !o.weight || !o.bias || !o.out) return fail("%s: null tensor", what);
    if (o.batch < 1 || o.in_channels < 1 || o.out_channels < 1 || o.height < 1 || o.width < 1)
        return fail("%s: bad shape (batch %d, in %d, out %d, %d x %d)", what, o.batch, o.in_channels, o.out_channels,
                    o.height, o.width);
    if (o.kernel_size < 1 || o.kernel_size > 7 || o.stride < 1 || o.stride > 2 || o.padding < 0 ||
        o.padding >= o.kernel_size)
        return fail("%s: unsupported kernel %d / stride %d / padding %d", what, o.kernel_size, o.stride, o.padding);
    if (o.x_nchw == 0 && o.in_channels % 32)
        return fail("%s: a channels-last input needs in_channels %% 32 == 0 (got %d)", what, o.in_channels);
    if (o.op != 0 && o.x_nchw) return fail("%s: the input is channels-last (x_nchw must be 0)", what);
    if (o.op == 2) {
        if (o.kernel_size != 3 || o.padding != 1)
            return fail("%s: kernel 3 with padding 1 only (got kernel %d, padding %d)", what, o.kernel_size, o.padding);
        if (o.out_channels % 8) return fail("%s: out_channels %% 8 == 0 (got %d)", what, o.out_channels);
        if (!o.offset_mask) return fail("%s: null offset / mask tensor", what);
        if (reinterpret_cast<uintptr_t>(o.offset_mask) & 15) return fail("%s: offset_mask must be 16-byte aligned", what);
    }
    if (o.op == 3 && o.residual) return fail("%s: takes no residual", what);
    if ((reinterpret_cast<uintptr_t>(o.x) | reinterpret_cast<uintptr_t>(o.weight)) & 15)
        return fail("%s: x and weight must be 16-byte aligned", what);
    const int ho = out_hw(o.height, o.kernel_size, o.stride, o.padding), wo = out_hw(o.width, o.kernel_size, o.stride, o.padding);
    if (ho < 1 || wo < 1) return fail("%s: empty output", what);
    const ConvGeom g = {o.x, o.weight, o.bias, o.residual, o.out, o.batch, o.in_channels, o.height, o.width, o.out_channels,
                        o.kernel_size, o.stride, o.padding, ho, wo, o.x_nchw, o.op == 2 ? 1 : o.splits};
    if (int rc = fill_conv(what, g, o.op == 3 ? 0 : precision, c)) return rc;
    if (o.op == 3 && precision == 1) c.x_bytes /= 2;   // the 16-bit activation under the three-plane weight
    c.out_nchw = o.out_nchw;
    c.relu = o.relu ? 1 : 0;
    c.om = o.op == 2 ? o.offset_mask : nullptr;
    return 0;
}

int run_conv(hipStream_t s, const sdetr_backbone_op &o, int precision, void *ws, int64_t ws_bytes)
{
    BConv c;
    if (int rc = make_conv(o, precision, c)) return rc;
    if (conv_workspace(c) > ws_bytes || (conv_workspace(c) && !ws))
        return fail("sdetr_backbone (conv): workspace of %lld bytes is too small (%lld needed)", (long long)ws_bytes,
                    (long long)conv_workspace(c));
    c.partial = reinterpret_cast<float *>(ws);
    const bool x3 = precision == 0;
    if (o.op == 2) {
        if (x3) launch_conv<true, kADeform, 0>(s, c);
        else launch_conv<false, kADeform, 0>(s, c);
        return check_launch("sdetr_backbone (deformable conv)");
    }
    if (o.op == 3) {
        if (x3) launch_conv<true, kANhwc, 0>(s, c);
        else launch_conv<true, kAWiden, 0>(s, c);
        return check_launch("sdetr_backbone (exact conv)");
    }
    if (x3 && o.x_nchw) launch_conv<true, kANchw, 0>(s, c);
    else if (x3) launch_conv<true, kANhwc, 0>(s, c);
    else if (o.x_nchw) launch_conv<false, kANchw, 0>(s, c);
    else launch_conv<false, kANhwc, 0>(s, c);
    return check_launch("sdetr_backbone (conv)");
}

// a max-pool op: x [batch, height, width, in_channels] -> out, both channels-last in the compute dtype
int check_maxpool(const sdetr_backbone_op &o, int precision)
{
    const char *what = "sdetr_backbone (max pool)";
    if (precision != 0 && precision != 1) return fail("%s: precision must be 0 or 1", what);
    if (!o.x || !o.out) return fail("%s: null tensor", what);
    if (o.batch < 1 || o.height < 1 || o.width < 1 || o.in_channels < 1 || o.in_channels % 8)
        return fail("%s: bad shape (batch %d, %d x %d, channels %d: a multiple of 8)", what, o.batch, o.height, o.width,
                    o.in_channels);
    if ((reinterpret_cast<uintptr_t>(o.x) | reinterpret_cast<uintptr_t>(o.out)) & 15)
        return fail("%s: tensors must be 16-byte aligned", what);
    return 0;
}

int run_maxpool(hipStream_t s, const sdetr_backbone_op &o, int precision)
{
    if (int rc = check_maxpool(o, precision)) return rc;
    const int batch = o.batch, h = o.height, w = o.width, c = o.in_channels;
    const int ho = out_hw(h, 3, 2, 1), wo = out_hw(w, 3, 2, 1);
    const int64_t total = (int64_t)batch * ho * wo * (c / (precision == 0 ? 4 : 8));
    const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 8192);
    if (precision == 0)
        hipLaunchKernelGGL(backbone_maxpool_kernel<true>, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const char *>(o.x),
                           batch, h, w, c, ho, wo, reinterpret_cast<char *>(o.out));
    else
        hipLaunchKernelGGL(backbone_maxpool_kernel<false>, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const char *>(o.x),
                           batch, h, w, c, ho, wo, reinterpret_cast<char *>(o.out));
    return check_launch("sdetr_backbone (max pool)");
}

// validation of one op without a launch; `need` receives its workspace bytes
int check_op(const sdetr_backbone_op &o, int precision, int64_t &need)
{
    need = 0;
    if (o.op == 0 || o.op == 2 || o.op == 3) {
        BConv c;
        if (int rc = make_conv(o, precision, c)) return rc;
        need = conv_workspace(c);
        return 0;
    }
    if (o.op == 1) return check_maxpool(o, precision);
    return fail("sdetr_backbone: unknown op kind %d", o.op);
}

int run_op(hipStream_t s, const sdetr_backbone_op &o, int precision, void *ws, int64_t ws_bytes)
{
    if (o.op == 0 || o.op == 2 || o.op == 3) return run_conv(s, o, precision, ws, ws_bytes);
    if (o.op == 1) return run_maxpool(s, o, precision);
    return fail("sdetr_backbone: unknown op kind %d", o.op);
}

using BackbonePlan = Plan<sdetr_backbone_op, check_op, run_op>;

}  // namespace
}  // namespace sdetr

using namespace sdetr;

extern "C" int64_t sdetr_backbone_packed_bytes(int out_channels, int in_channels, int kernel_size, int precision)
{
    if (out_channels < 1 || in_channels < 1 || kernel_size < 1 || (precision != 0 && precision != 1)) return -1;
    return (int64_t)(precision == 0 ? 3 : 1) * out_channels * round32(in_channels * kernel_size * kernel_size) * 2;
}

extern "C" int sdetr_backbone_pack(sdetr_stream_t stream, const float *weight, const float *gamma, const float *beta,
                                   const float *running_mean, const float *running_var, float eps, int out_channels,
                                   int in_channels, int kernel_size, int layout, int precision, void *packed, float *bias)
{
    if (!weight || !gamma || !beta || !running_mean || !running_var || !packed || !bias)
        return fail("sdetr_backbone_pack: null tensor");
    if (sdetr_backbone_packed_bytes(out_channels, in_channels, kernel_size, precision) < 0 || (layout != 0 && layout != 1))
        return fail("sdetr_backbone_pack: bad arguments (out %d, in %d, kernel %d, layout %d, precision %d)", out_channels,
                    in_channels, kernel_size, layout, precision);
    const int kpad = round32(in_channels * kernel_size * kernel_size);
    const int64_t total = (int64_t)out_channels * kpad;
    const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(backbone_pack_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, weight, gamma, beta,
                       running_mean, running_var, eps, out_channels, in_channels, kernel_size, kpad, layout, precision,
                       reinterpret_cast<uint16_t *>(packed), bias);
    return check_launch("sdetr_backbone_pack");
}

extern "C" int sdetr_backbone_conv_splits(const sdetr_backbone_op *op, int precision)
{
    BConv c;
    if (!op || (op->op != 0 && op->op != 2 && op->op != 3)) return fail("sdetr_backbone_conv_splits: not a conv op");
    if (make_conv(*op, precision, c)) return SDETR_EINVAL;
    return c.splits;
}

extern "C" int64_t sdetr_backbone_workspace_bytes(const sdetr_backbone_op *ops, int n_ops, int precision)
{
    return BackbonePlan::workspace_bytes(ops, n_ops, precision);
}

extern "C" int sdetr_backbone_conv(sdetr_stream_t stream, const sdetr_backbone_op *op, int precision, void *workspace,
                                   int64_t workspace_bytes)
{
    if (!op || (op->op != 0 && op->op != 2 && op->op != 3)) return fail("sdetr_backbone_conv: not a conv op");
    return run_op((hipStream_t)stream, *op, precision, workspace, workspace_bytes);
}

extern "C" int sdetr_backbone_maxpool(sdetr_stream_t stream, const void *x, int batch, int height, int width, int channels,
                                      int precision, void *out)
{
    sdetr_backbone_op o = {};
    o.op = 1;
    o.x = x;
    o.out = out;
    o.batch = batch;
    o.height = height;
    o.width = width;
    o.in_channels = o.out_channels = channels;
    return run_op((hipStream_t)stream, o, precision, nullptr, 0);
}

extern "C" int sdetr_backbone_run(sdetr_stream_t stream, const sdetr_backbone_op *ops, int n_ops, int precision,
                                  void *workspace, int64_t workspace_bytes)
{
    return BackbonePlan::run("sdetr_backbone", stream, ops, n_ops, precision, workspace, workspace_bytes);
}

extern "C" int sdetr_backbone_batch_images_ex(sdetr_stream_t stream, const void *const *images, const int *image_hw,
                                              int batch, int is_uint8, int normalize, int canvas_height, int canvas_width,
                                              float *canvas, uint8_t *mask)
{
    if (!images || !image_hw || !canvas || !mask) return fail("sdetr_backbone_batch_images: null argument");
    if (batch < 1 || batch > kBMaxImages) return fail("sdetr_backbone_batch_images: 1 .. %d images (got %d)", kBMaxImages, batch);
    BatchArgs a;
    for (int b = 0; b < batch; ++b) {
        const int h = image_hw[2 * b], w = image_hw[2 * b + 1];
        if (!images[b] || h < 1 || w < 1 || h > canvas_height || w > canvas_width)
            return fail("sdetr_backbone_batch_images: image %d (%d x %d) does not fit the %d x %d canvas", b, h, w,
                        canvas_height, canvas_width);
        a.img[b] = images[b];
        a.h[b] = h;
        a.w[b] = w;
    }
    a.batch = batch;
    a.hp = canvas_height;
    a.wp = canvas_width;
    a.is_u8 = is_uint8 ? 1 : 0;
    a.normalize = normalize ? 1 : 0;
    a.canvas = canvas;
    a.mask = mask;
    const int64_t total = (int64_t)batch * canvas_height * canvas_width;
    const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(backbone_batch_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("sdetr_backbone_batch_images");
}

extern "C" int sdetr_backbone_batch_images(sdetr_stream_t stream, const void *const *images, const int *image_hw, int batch,
                                           int is_uint8, int canvas_height, int canvas_width, float *canvas, uint8_t *mask)
{
    return sdetr_backbone_batch_images_ex(stream, images, image_hw, batch, is_uint8, 1, canvas_height, canvas_width, canvas,
                                          mask);
}

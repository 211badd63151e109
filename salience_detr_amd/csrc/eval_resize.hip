// EvalResize (models/detectors/base_detector.py:20-53, transforms/_functional_tensor.py:439-474): the antialiased
// bilinear resize in front of the eval transform, F.interpolate(img[None], size=(nh, nw), mode="bilinear",
// align_corners=False, antialias=True).
//
// Per axis: scale = in / out (fp32), support = max(scale, 1); output i takes the input taps [lo, lo + n) around
// center = scale * (i + 0.5) with the triangle weight 1 - |(tap + 0.5 - center) / support|, renormalised to sum 1 (which is
// what handles the borders).  The horizontal sum of every tap row is taken first, then the vertical sum of those, as the
// framework's two passes do.
//
// Two launches share resized_pixel() (resize_core.h, also the training transform's), the ONE routine for a pixel's value:
//   * eval_resize_kernel<T, false>: [3, h, w] -> tightly packed [3, nh, nw] of the same type (u8: round half to even);
//   * eval_resize_kernel<T, true>: the same value (+ for u8 that rounding, then / 255) -> Normalize -> the zero-padded
//     canvas and the padding mask of sdetr_backbone_batch_images_ex, every element written by this launch.
// A workgroup owns a 64 x 4 tile of output pixels (one wave per row, coalesced along the width).  Its 64 column taps and
// 4 row taps (first tap, count, centre, normalisation) are built once into LDS; the weights themselves are a handful of
// VALU operations per tap, recomputed from that entry, so the tap count -- which grows with the shrink factor -- is
// a loop bound and not a table size: any factor runs.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "image_norm.h"
#include "resize_core.h"

namespace sdetr {
namespace {

struct ResizeArgs {
    const void *img[kRMaxImages];
    void *out[kRMaxImages];          // resize only
    int h[kRMaxImages], w[kRMaxImages], nh[kRMaxImages], nw[kRMaxImages];
    int batch, hp, wp;               // fused: the canvas; resize only: the largest output (the grid's extent)
    float *canvas;
    uint8_t *mask;
};

template <typename T, bool FUSED>
__global__ void __launch_bounds__(kRTileW * kRTileH) eval_resize_kernel(ResizeArgs a)
{
    __shared__ AxisTap s_x[kRTileW], s_y[kRTileH];
    const int tiles_x = (a.wp + kRTileW - 1) / kRTileW, tiles_y = (a.hp + kRTileH - 1) / kRTileH;
    const int b = (int)(blockIdx.x / (unsigned)(tiles_x * tiles_y));
    const int r = (int)(blockIdx.x - (unsigned)b * (unsigned)(tiles_x * tiles_y));
    const int y0 = r / tiles_x * kRTileH, x0 = (r - r / tiles_x * tiles_x) * kRTileW;
    const int h = a.h[b], w = a.w[b], nh = a.nh[b], nw = a.nw[b];
    const int tid = threadIdx.x, lx = tid & (kRTileW - 1), ly = tid / kRTileW;
    const bool tile_has_image = y0 < nh && x0 < nw;          // block-uniform
    if (!FUSED && !tile_has_image) return;
    if (tile_has_image) {
        if (tid < kRTileW) {
            if (x0 + tid < nw) s_x[tid] = axis_tap(x0 + tid, w, nw);
        } else if (tid < kRTileW + kRTileH) {
            if (y0 + tid - kRTileW < nh) s_y[tid - kRTileW] = axis_tap(y0 + tid - kRTileW, h, nh);
        }
    }
    __syncthreads();
    const int oy = y0 + ly, ox = x0 + lx;
    const bool in = oy < nh && ox < nw;
    float v[3] = {0.f, 0.f, 0.f};
    if (in) resized_pixel<std::is_same<T, uint8_t>::value>(planar_source<T>(a.img[b], h, w, false), s_y[ly], s_x[lx], v);
    if (FUSED) {
        if (oy >= a.hp || ox >= a.wp) return;
        const int64_t plane = (int64_t)a.hp * a.wp, p = (int64_t)oy * a.wp + ox;
        for (int ch = 0; ch < 3; ++ch) {
            float c = 0.f;
            if (in) c = image_normalize(std::is_same<T, uint8_t>::value ? image_unit_from_u8(v[ch]) : v[ch], ch);
            a.canvas[((int64_t)b * 3 + ch) * plane + p] = c;
        }
        a.mask[(int64_t)b * plane + p] = in ? 0 : 1;
    } else if (in) {
        T *out = reinterpret_cast<T *>(a.out[b]);
        for (int ch = 0; ch < 3; ++ch) out[((int64_t)ch * nh + oy) * nw + ox] = (T)v[ch];
    }
}

// the arguments both entry points share; `what` names the caller in the error text
int fill_args(const char *what, const void *const *images, const int *image_hw, const int *out_hw, int batch, ResizeArgs &a)
{
    if (!images || !image_hw || !out_hw) return fail("%s: null argument", what);
    if (batch < 1 || batch > kRMaxImages) return fail("%s: 1 .. %d images (got %d)", what, kRMaxImages, batch);
    for (int b = 0; b < batch; ++b) {
        const int h = image_hw[2 * b], w = image_hw[2 * b + 1], nh = out_hw[2 * b], nw = out_hw[2 * b + 1];
        if (!images[b]) return fail("%s: image %d is null", what, b);
        if (h < 1 || w < 1 || nh < 1 || nw < 1 || h > kRMaxSide || w > kRMaxSide || nh > kRMaxSide || nw > kRMaxSide)
            return fail("%s: image %d (%d x %d -> %d x %d): every side must be 1 .. %d", what, b, h, w, nh, nw, kRMaxSide);
        a.img[b] = images[b];
        a.out[b] = nullptr;
        a.h[b] = h;
        a.w[b] = w;
        a.nh[b] = nh;
        a.nw[b] = nw;
    }
    a.batch = batch;
    a.canvas = nullptr;
    a.mask = nullptr;
    return 0;
}

// number of workgroups for a.hp x a.wp tiles per image, or -1 (with the error set)
int64_t grid_blocks(const char *what, const ResizeArgs &a)
{
    const int64_t blocks = (int64_t)a.batch * ((a.hp + kRTileH - 1) / kRTileH) * ((a.wp + kRTileW - 1) / kRTileW);
    if (blocks >= (int64_t(1) << 31)) {
        fail("%s: %lld workgroups do not fit one launch", what, (long long)blocks);
        return -1;
    }
    return blocks;
}

}  // namespace
}  // namespace sdetr

using namespace sdetr;

extern "C" int sdetr_backbone_resize_images(sdetr_stream_t stream, const void *const *images, const int *image_hw,
                                            const int *out_hw, int batch, int is_uint8, void *const *outputs)
{
    const char *what = "sdetr_backbone_resize_images";
    ResizeArgs a;
    if (!outputs) return fail("%s: null argument", what);
    if (fill_args(what, images, image_hw, out_hw, batch, a)) return SDETR_EINVAL;
    a.hp = a.wp = 1;
    for (int b = 0; b < batch; ++b) {
        if (!outputs[b]) return fail("%s: output %d is null", what, b);
        a.out[b] = outputs[b];
        a.hp = std::max(a.hp, a.nh[b]);
        a.wp = std::max(a.wp, a.nw[b]);
    }
    const int64_t blocks = grid_blocks(what, a);
    if (blocks < 0) return SDETR_EINVAL;
    if (is_uint8)
        hipLaunchKernelGGL((eval_resize_kernel<uint8_t, false>), dim3((unsigned)blocks), dim3(kRTileW * kRTileH), 0,
                           (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((eval_resize_kernel<float, false>), dim3((unsigned)blocks), dim3(kRTileW * kRTileH), 0,
                           (hipStream_t)stream, a);
    return check_launch(what);
}

extern "C" int sdetr_backbone_resize_batch_images(sdetr_stream_t stream, const void *const *images, const int *image_hw,
                                                  const int *out_hw, int batch, int is_uint8, int canvas_height,
                                                  int canvas_width, float *canvas, uint8_t *mask)
{
    const char *what = "sdetr_backbone_resize_batch_images";
    ResizeArgs a;
    if (!canvas || !mask) return fail("%s: null argument", what);
    if (fill_args(what, images, image_hw, out_hw, batch, a)) return SDETR_EINVAL;
    if (canvas_height < 1 || canvas_width < 1 || canvas_height > kRMaxSide || canvas_width > kRMaxSide)
        return fail("%s: bad canvas %d x %d", what, canvas_height, canvas_width);
    for (int b = 0; b < batch; ++b)
        if (a.nh[b] > canvas_height || a.nw[b] > canvas_width)
            return fail("%s: image %d resized to %d x %d does not fit the %d x %d canvas", what, b, a.nh[b], a.nw[b],
                        canvas_height, canvas_width);
    a.hp = canvas_height;
    a.wp = canvas_width;
    a.canvas = canvas;
    a.mask = mask;
    const int64_t blocks = grid_blocks(what, a);
    if (blocks < 0) return SDETR_EINVAL;
    if (is_uint8)
        hipLaunchKernelGGL((eval_resize_kernel<uint8_t, true>), dim3((unsigned)blocks), dim3(kRTileW * kRTileH), 0,
                           (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((eval_resize_kernel<float, true>), dim3((unsigned)blocks), dim3(kRTileW * kRTileH), 0,
                           (hipStream_t)stream, a);
    return check_launch(what);
}

// The training transform's image half (transforms/presets.py `detr`, `multiscale`, `hflip`; transforms/v2/_geometry.py
// RandomShortestSize, transforms/crop.py RandomSizeCrop, applied to tensors): horizontal flip -> resize -> crop -> resize ->
// ConvertImageDtype -> Normalize -> zero padding + padding mask, ONE launch per batch.  The draws and the boxes are host
// work (train_transform.py); this launch gets every image's plan: the flip, the number of resizes (0, 1 or 2), the size
// after the first, the crop inside it, the final size.
//
// Every value comes from resized_pixel() (resize_core.h), the routine EvalResize is pinned with, so the canvas equals,
// bit for bit, sdetr_backbone_batch_images of the images built step by step with sdetr_backbone_resize_images.
//
//   * flip 1 mirrors the SOURCE: column x is read from w - 1 - x and the taps are those of the mirrored image (a resize
//     and its mirror image do not agree bit for bit: tap centres and the summation order do not mirror in fp32).
//     flip 2 mirrors the RESULT of a one-resize plan (the `multiscale` preset resizes first): output column x takes
//     the taps of column nw - 1 - x.
//   * 0 or 1 resizes: the fused EvalResize kernel's tile (64 x 4 output pixels, taps built once into LDS) with that read.
//   * 2 resizes: phase 1 stages into LDS the window of intermediate pixels the tile's second-resize taps cover -- window
//     pixel (y, x) of the crop is the first resize evaluated at (top + y, left + x) of the h1 x w1 image, which never
//     exists in memory; u8: rounded half to even and clamped, as the reference's cast round trip -- and phase 2 forms the
//     output from LDS with the second resize's taps (u8: rounded again), converts and normalises.  Intermediate pixels
//     outside the crop are never computed.  The window holds kWinH x kWinW pixels: every second resize that shrinks by
//     up to 1.25 (the `detr` preset's extreme, 600 / 480) stages.  A tile whose window is larger (a strong second
//     shrink) recomputes the intermediate pixel at every tap instead -- slow and correct, any factor runs.  The choice is
//     block-uniform; sdetr_backbone_train_plan_stats tells on the host which tiles of a plan take which.
#include <algorithm>
#include <type_traits>

#include "common.h"
#include "image_norm.h"
#include "resize_core.h"

namespace sdetr {
namespace {

// 64 outputs at scale 1.25: 63 * 1.25 + 2 * 1.25 + 2 < 84 columns; 4 rows: 3 * 1.25 + 2 * 1.25 + 2 < 9 rows
constexpr int kWinW = 96, kWinH = 12;
constexpr int kPlanInts = 10;        // flip, n_stages, h1, w1, top, left, ch, cw, nh, nw

struct TrainArgs {
    const void *img[kRMaxImages];
    int h[kRMaxImages], w[kRMaxImages];
    int mode[kRMaxImages];           // flip | n_stages << 2
    int h1[kRMaxImages], w1[kRMaxImages], top[kRMaxImages], left[kRMaxImages], ch[kRMaxImages], cw[kRMaxImages];
    int nh[kRMaxImages], nw[kRMaxImages];
    int batch, hp, wp;
    float *canvas;
    uint8_t *mask;
};

// the staged window of intermediate pixels: (y, x) in the crop's coordinates
struct WindowSource {
    const float *win;
    int y0, x0;
    __device__ __forceinline__ void load(int y, int x, float s[3]) const
    {
        const float *p = win + (y - y0) * kWinW + (x - x0);
        for (int ch = 0; ch < 3; ++ch) s[ch] = p[ch * kWinH * kWinW];
    }
};

// the same pixels without a window: the first resize evaluated at every read
template <typename T>
struct RecomputeSource {
    PlanarSource<T> src;
    int h, w, h1, w1, top, left;
    __device__ void load(int y, int x, float s[3]) const
    {
        const AxisTap ty = axis_tap(top + y, h, h1), tx = axis_tap(left + x, w, w1);
        resized_pixel<std::is_same<T, uint8_t>::value>(src, ty, tx, s);
    }
};

// [first, last) of the input taps that outputs [o0, o0 + count) of an axis read (the spans are monotone in the index)
__host__ __device__ inline void window_of(int o0, int count, int in, int out, int &first, int &last)
{
    int lo, n;
    axis_span(o0, in, out, first, n);
    axis_span(o0 + count - 1, in, out, lo, n);
    last = lo + n;
}

template <typename T>
__global__ void __launch_bounds__(kRTileW * kRTileH) train_transform_kernel(TrainArgs a)
{
    constexpr bool ROUND = std::is_same<T, uint8_t>::value;
    __shared__ AxisTap s_x[kRTileW], s_y[kRTileH];       // the last resize's taps of the tile
    __shared__ AxisTap s_wx[kWinW], s_wy[kWinH];         // the first resize's taps of the window
    __shared__ float s_win[3 * kWinH * kWinW];
    const int tiles_x = (a.wp + kRTileW - 1) / kRTileW, tiles_y = (a.hp + kRTileH - 1) / kRTileH;
    const int b = (int)(blockIdx.x / (unsigned)(tiles_x * tiles_y));
    const int r = (int)(blockIdx.x - (unsigned)b * (unsigned)(tiles_x * tiles_y));
    const int y0 = r / tiles_x * kRTileH, x0 = (r - r / tiles_x * tiles_x) * kRTileW;
    const int h = a.h[b], w = a.w[b], nh = a.nh[b], nw = a.nw[b], flip = a.mode[b] & 3;
    const bool two = (a.mode[b] >> 2) == 2;
    // what the last resize reads: the crop, or the image itself
    const int in_h = two ? a.ch[b] : h, in_w = two ? a.cw[b] : w;
    const int tid = threadIdx.x, lx = tid & (kRTileW - 1), ly = tid / kRTileW;
    const int oy = y0 + ly, ox = x0 + lx;
    const bool in = oy < nh && ox < nw;
    const PlanarSource<T> src = planar_source<T>(a.img[b], h, w, flip == 1);
    float v[3] = {0.f, 0.f, 0.f};
    if (y0 < nh && x0 < nw) {                            // block-uniform: the tile has pixels of the image
        if (tid < kRTileW) {
            if (x0 + tid < nw) s_x[tid] = axis_tap(flip == 2 ? nw - 1 - (x0 + tid) : x0 + tid, in_w, nw);
        } else if (tid < kRTileW + kRTileH) {
            if (y0 + tid - kRTileW < nh) s_y[tid - kRTileW] = axis_tap(y0 + tid - kRTileW, in_h, nh);
        }
        __syncthreads();
        if (!two) {
            if (in) resized_pixel<ROUND>(src, s_y[ly], s_x[lx], v);
        } else {
            const int h1 = a.h1[b], w1 = a.w1[b], top = a.top[b], left = a.left[b];
            const int last_x = min(kRTileW, nw - x0) - 1, last_y = min(kRTileH, nh - y0) - 1;
            const int wx0 = s_x[0].lo, wy0 = s_y[0].lo;
            const int win_w = s_x[last_x].lo + s_x[last_x].n - wx0, win_h = s_y[last_y].lo + s_y[last_y].n - wy0;
            if (win_w <= kWinW && win_h <= kWinH) {      // block-uniform
                if (tid < win_w) s_wx[tid] = axis_tap(left + wx0 + tid, w, w1);
                else if (tid >= 128 && tid - 128 < win_h) s_wy[tid - 128] = axis_tap(top + wy0 + tid - 128, h, h1);
                __syncthreads();
                for (int p = tid; p < win_h * win_w; p += kRTileW * kRTileH) {
                    const int py = p / win_w, px = p - py * win_w;
                    float s[3];
                    resized_pixel<ROUND>(src, s_wy[py], s_wx[px], s);
                    for (int ch = 0; ch < 3; ++ch) s_win[(ch * kWinH + py) * kWinW + px] = s[ch];
                }
                __syncthreads();
                if (in) resized_pixel<ROUND>(WindowSource{s_win, wy0, wx0}, s_y[ly], s_x[lx], v);
            } else if (in) {
                resized_pixel<ROUND>(RecomputeSource<T>{src, h, w, h1, w1, top, left}, s_y[ly], s_x[lx], v);
            }
        }
    }
    if (oy >= a.hp || ox >= a.wp) return;
    const int64_t plane = (int64_t)a.hp * a.wp, p = (int64_t)oy * a.wp + ox;
    for (int ch = 0; ch < 3; ++ch) {
        float c = 0.f;
        if (in) c = image_normalize(ROUND ? image_unit_from_u8(v[ch]) : v[ch], ch);
        a.canvas[((int64_t)b * 3 + ch) * plane + p] = c;
    }
    a.mask[(int64_t)b * plane + p] = in ? 0 : 1;
}

bool side_ok(int v) { return v >= 1 && v <= kRMaxSide; }

// the checks of one image's plan (everything but the pointers and the canvas); 0 or the error
int check_plan(const char *what, int b, int h, int w, const int *p)
{
    const int flip = p[0], stages = p[1], h1 = p[2], w1 = p[3], top = p[4], left = p[5], ch = p[6], cw = p[7], nh = p[8], nw = p[9];
    if (!side_ok(h) || !side_ok(w) || !side_ok(nh) || !side_ok(nw))
        return fail("%s: image %d (%d x %d -> %d x %d): every side must be 1 .. %d", what, b, h, w, nh, nw, kRMaxSide);
    if (stages < 0 || stages > 2) return fail("%s: image %d: n_stages must be 0, 1 or 2 (got %d)", what, b, stages);
    if (flip < 0 || flip > 2 || (flip == 2 && stages == 2))
        return fail("%s: image %d: flip must be 0, 1 (the source mirrored) or, with at most one resize, 2 (the result "
                    "mirrored); got %d with n_stages %d", what, b, flip, stages);
    if (stages == 0 && (nh != h || nw != w))
        return fail("%s: image %d: n_stages 0 keeps the size %d x %d (got %d x %d)", what, b, h, w, nh, nw);
    if (stages == 2) {
        if (!side_ok(h1) || !side_ok(w1))
            return fail("%s: image %d: intermediate size %d x %d: every side must be 1 .. %d", what, b, h1, w1, kRMaxSide);
        if (top < 0 || left < 0 || ch < 1 || cw < 1 || ch > h1 - top || cw > w1 - left)
            return fail("%s: image %d: the crop (top %d, left %d, %d x %d) does not lie inside the %d x %d intermediate image",
                        what, b, top, left, ch, cw, h1, w1);
    }
    return 0;
}

}  // namespace
}  // namespace sdetr

using namespace sdetr;

extern "C" int sdetr_backbone_train_batch_images(sdetr_stream_t stream, const void *const *images, const int *image_hw,
                                                 const int *plan, int batch, int is_uint8, int canvas_height,
                                                 int canvas_width, float *canvas, uint8_t *mask)
{
    const char *what = "sdetr_backbone_train_batch_images";
    TrainArgs a;
    if (!images || !image_hw || !plan || !canvas || !mask) return fail("%s: null argument", what);
    if (batch < 1 || batch > kRMaxImages) return fail("%s: 1 .. %d images (got %d)", what, kRMaxImages, batch);
    if (canvas_height < 1 || canvas_width < 1 || canvas_height > kRMaxSide || canvas_width > kRMaxSide)
        return fail("%s: bad canvas %d x %d", what, canvas_height, canvas_width);
    for (int b = 0; b < batch; ++b) {
        const int *p = plan + (size_t)b * kPlanInts;
        if (!images[b]) return fail("%s: image %d is null", what, b);
        if (check_plan(what, b, image_hw[2 * b], image_hw[2 * b + 1], p)) return SDETR_EINVAL;
        if (p[8] > canvas_height || p[9] > canvas_width)
            return fail("%s: image %d transformed to %d x %d does not fit the %d x %d canvas", what, b, p[8], p[9],
                        canvas_height, canvas_width);
        a.img[b] = images[b];
        a.h[b] = image_hw[2 * b];
        a.w[b] = image_hw[2 * b + 1];
        a.mode[b] = p[0] | p[1] << 2;
        a.h1[b] = p[2];
        a.w1[b] = p[3];
        a.top[b] = p[4];
        a.left[b] = p[5];
        a.ch[b] = p[6];
        a.cw[b] = p[7];
        a.nh[b] = p[8];
        a.nw[b] = p[9];
    }
    a.batch = batch;
    a.hp = canvas_height;
    a.wp = canvas_width;
    a.canvas = canvas;
    a.mask = mask;
    const int64_t blocks = (int64_t)batch * ((a.hp + kRTileH - 1) / kRTileH) * ((a.wp + kRTileW - 1) / kRTileW);
    if (blocks >= (int64_t(1) << 31)) return fail("%s: %lld workgroups do not fit one launch", what, (long long)blocks);
    if (is_uint8)
        hipLaunchKernelGGL((train_transform_kernel<uint8_t>), dim3((unsigned)blocks), dim3(kRTileW * kRTileH), 0,
                           (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((train_transform_kernel<float>), dim3((unsigned)blocks), dim3(kRTileW * kRTileH), 0,
                           (hipStream_t)stream, a);
    return check_launch(what);
}

extern "C" int sdetr_backbone_train_plan_stats(const int *image_hw, const int *plan, int batch, int64_t *staged,
                                               int64_t *recomputed)
{
    const char *what = "sdetr_backbone_train_plan_stats";
    if (!image_hw || !plan || !staged || !recomputed) return fail("%s: null argument", what);
    if (batch < 1 || batch > kRMaxImages) return fail("%s: 1 .. %d images (got %d)", what, kRMaxImages, batch);
    *staged = *recomputed = 0;
    for (int b = 0; b < batch; ++b) {
        const int *p = plan + (size_t)b * kPlanInts;
        if (check_plan(what, b, image_hw[2 * b], image_hw[2 * b + 1], p)) return SDETR_EINVAL;
        if (p[1] != 2) continue;
        const int ch = p[6], cw = p[7], nh = p[8], nw = p[9];
        // a tile's window is as wide as its column of tiles makes it and as high as its row of tiles does
        int64_t fit_x = 0, fit_y = 0;
        const int64_t tiles_x = (nw + kRTileW - 1) / kRTileW, tiles_y = (nh + kRTileH - 1) / kRTileH;
        for (int x0 = 0, first, last; x0 < nw; x0 += kRTileW) {
            window_of(x0, std::min(kRTileW, nw - x0), cw, nw, first, last);
            fit_x += last - first <= kWinW;
        }
        for (int y0 = 0, first, last; y0 < nh; y0 += kRTileH) {
            window_of(y0, std::min(kRTileH, nh - y0), ch, nh, first, last);
            fit_y += last - first <= kWinH;
        }
        *staged += fit_x * fit_y;
        *recomputed += tiles_x * tiles_y - fit_x * fit_y;
    }
    return 0;
}

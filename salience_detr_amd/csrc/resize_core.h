// The antialiased bilinear resize's per-pixel routine, F.interpolate(..., mode="bilinear", align_corners=False,
// antialias=True), shared by EvalResize (eval_resize.hip) and the training transform (train_transform.hip) so that the
// two cannot drift apart: both call resized_pixel(), the ONE routine for a pixel's value.
//
// Per axis: scale = in / out (fp32), support = max(scale, 1); output i takes the input taps [lo, lo + n) around
// center = scale * (i + 0.5) with the triangle weight 1 - |(tap + 0.5 - center) / support|, renormalised to sum 1 (which is
// what handles the borders).  The horizontal sum of every tap row is taken first, then the vertical sum of those, as the
// framework's two passes do.
//
// resized_pixel() reads its taps through a source: anything with `load(y, x, float s[3])`, the three channels of the
// input pixel (y, x) as floats.  PlanarSource is an image in memory ([3, h, w], optionally read mirrored along the
// width); train_transform.hip adds a window of intermediate pixels in LDS and a source that recomputes them.
#pragma once

#include "common.h"

namespace sdetr {

constexpr int kRMaxImages = 64;
constexpr int kRTileW = 64, kRTileH = 4;
constexpr int kRMaxSide = 1 << 24;   // tap indices are exact in fp32 up to here

struct AxisTap {
    int lo, n;
    float center, norm, invscale;
};

__device__ __forceinline__ float triangle(float x)
{
    x = fabsf(x);
    return x < 1.f ? 1.f - x : 0.f;
}

// un-normalised weight of tap j of an entry
__device__ __forceinline__ float raw_weight(const AxisTap &t, int j)
{
    return triangle(((float)(t.lo + j) - t.center + 0.5f) * t.invscale);
}

__device__ __forceinline__ float tap_weight(const AxisTap &t, int j) { return raw_weight(t, j) * t.norm; }

// the taps [lo, lo + n) of output index i on an axis of `in` -> `out` samples (host and device: the host uses it to
// tell which workgroups of a plan stage their window); returns the centre
__host__ __device__ inline float axis_span(int i, int in, int out, int &lo, int &n)
{
    const float scale = (float)in / (float)out;
    const float support = scale >= 1.f ? scale : 1.f;
    const float at = (float)i + 0.5f, center = scale * at;
    // center -+ support, each as ONE fused operation (what the compiler makes of `scale * at - support` on the device;
    // spelled out so that the host agrees); the half is added in double and truncated, as the framework does
    const int max_taps = (int)ceilf(support) * 2 + 1;
    const int first = (int)((double)fmaf(scale, at, -support) + 0.5), last = (int)((double)fmaf(scale, at, support) + 0.5);
    lo = first > 0 ? first : 0;
    const int span = (last < in ? last : in) - lo;
    n = span < 0 ? 0 : (span < max_taps ? span : max_taps);
    return center;
}

// the window of output index i on an axis of `in` -> `out` samples
__device__ inline AxisTap axis_tap(int i, int in, int out)
{
    const float scale = (float)in / (float)out;
    AxisTap t;
    t.invscale = scale >= 1.f ? 1.f / scale : 1.f;
    t.center = axis_span(i, in, out, t.lo, t.n);
    float total = 0.f;
    for (int j = 0; j < t.n; ++j) total += raw_weight(t, j);
    t.norm = total != 0.f ? 1.f / total : 1.f;
    return t;
}

// an image [3, h, w] in memory; `mirrored`: pixel (y, x) is read from column w - 1 - x (image.flip(-1), never built)
template <typename T>
struct PlanarSource {
    const T *img;
    int w;
    int64_t plane;
    bool mirrored;
    __device__ __forceinline__ void load(int y, int x, float s[3]) const
    {
        const T *p = img + (int64_t)y * w + (mirrored ? w - 1 - x : x);
        for (int ch = 0; ch < 3; ++ch) s[ch] = (float)p[ch * plane];
    }
};

template <typename T>
__device__ __forceinline__ PlanarSource<T> planar_source(const void *img, int h, int w, bool mirrored)
{
    return PlanarSource<T>{reinterpret_cast<const T *>(img), w, (int64_t)h * w, mirrored};
}

// The resized value of the three channels of one output pixel, as a float of the image's own type: with ROUND (u8) the
// sum over the 0..255 values rounded half to even (torch.round + the cast back).  Zero-weight taps are skipped, so an
// output whose size equals the input's is the input bit for bit.
template <bool ROUND, typename Source>
__device__ __forceinline__ void resized_pixel(const Source &src, const AxisTap &ty, const AxisTap &tx, float v[3])
{
    float acc[3] = {0.f, 0.f, 0.f};
    bool first_row = true;
    for (int j = 0; j < ty.n; ++j) {
        const float wy = tap_weight(ty, j);
        if (wy == 0.f) continue;
        float t[3] = {0.f, 0.f, 0.f};
        bool first = true;
        for (int i = 0; i < tx.n; ++i) {
            const float wx = tap_weight(tx, i);
            if (wx == 0.f) continue;
            float s[3];
            src.load(ty.lo + j, tx.lo + i, s);
            for (int ch = 0; ch < 3; ++ch) t[ch] = first ? __fmul_rn(s[ch], wx) : fmaf(s[ch], wx, t[ch]);
            first = false;
        }
        for (int ch = 0; ch < 3; ++ch) acc[ch] = first_row ? __fmul_rn(t[ch], wy) : fmaf(t[ch], wy, acc[ch]);
        first_row = false;
    }
    for (int ch = 0; ch < 3; ++ch) v[ch] = ROUND ? fminf(fmaxf(rintf(acc[ch]), 0.f), 255.f) : acc[ch];
}

}  // namespace sdetr

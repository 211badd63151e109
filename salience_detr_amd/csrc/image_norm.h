// The eval transform's per-pixel arithmetic (ConvertImageDtype + Normalize, models/detectors/base_detector.py:73-74),
// shared by the batching kernel (backbone.hip) and the fused resize + batching kernel (eval_resize.hip) so that the two
// cannot drift apart: a canvas built from pre-resized images equals the fused one bit for bit.
#pragma once

#include "common.h"

namespace sdetr {

// u8 -> [0, 1] as ConvertImageDtype does (v / 255 in fp32)
__device__ __forceinline__ float image_unit_from_u8(float v) { return v / 255.f; }

// (v - mean[ch]) / std[ch] with the ImageNet statistics: subtract, then divide (IEEE, as the reference's sub_ / div_)
__device__ __forceinline__ float image_normalize(float v, int ch)
{
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    return (v - mean[ch]) / sd[ch];
}

}  // namespace sdetr

// The exact (erf) GELU shared by the salience head (salience_head_core.h) and the ConvNeXt MLP epilogue
// (backbone_conv_core.h).  Every statement is an explicit fmaf or a single operation, so the value does not depend on the
// including file's fp-contract setting.
#pragma once
#include "common.h"

namespace sdetr {

// GELU (erf form, torch.nn.GELU()'s default).  Round 6: erf(t) = 1 - 2^(-t p(t)), t = |x| / sqrt 2, p of degree 7 fitted to
// -log2(erfc(t)) / t on [0, 4] (weights = the error of erf per error of p; benchmarks/fit_erf.py): max |error| 8.3e-8 over
// [0, 6] in fp32 arithmetic -- the rounding of a result next to 1 -- and 0 / 1 beyond (p stays positive).  14 vector
// instructions + v_exp_f32 where the library's erff is ~60 with both of its branches taken by a mixed wave: cycle
// stamps put 9 500 of stage 2's 33 700 cycles per workgroup in 32 erff per lane.  |gelu error| <= 0.5 |x| 1e-7.
__device__ __forceinline__ float erf_pos(float t)   // t >= 0
{
    float p = 4.535823973128572e-05f;
    p = fmaf(p, t, -0.00044550452730618417f);
    p = fmaf(p, t, 0.0014894308988004923f);
    p = fmaf(p, t, 0.0007746480405330658f);
    p = fmaf(p, t, -0.028253698721528053f);
    p = fmaf(p, t, 0.14848162233829498f);
    p = fmaf(p, t, 0.9184163808822632f);
    p = fmaf(p, t, 1.6279085874557495f);
    return 1.f - __builtin_amdgcn_exp2f(-t * p);
}
__device__ __forceinline__ float gelu_erf(float x)
{
#ifdef SH_LIB_ERF
    return 0.5f * x * (1.f + erff(x * 0.70710678118654752440f));
#else
    const float e = erf_pos(fabsf(x) * 0.70710678118654752440f);
    const float h = 0.5f * x;
    return fmaf(fabsf(h), e, h);   // 0.5 x (1 + sign(x) erf(|x| / sqrt 2))
#endif
}

}  // namespace sdetr

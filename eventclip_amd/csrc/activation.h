// Exact GELU, x * Phi(x) (torch.nn.GELU(), open_clip's CLIPs without a -quickgelu suffix, Hugging Face
// hidden_act "gelu"), for the GEMM epilogues (gemm.hip, forward and training) and the split row kernel
// (layernorm.hip).  QuickGELU, the default everywhere, stays where it was in those files.
//
// Phi comes from Abramowitz & Stegun 7.1.26,
//     erfc(z) = t (a1 + t (a2 + t (a3 + t (a4 + t a5)))) exp(-z^2) + eps(z),  t = 1 / (1 + p z),  |eps| <= 1.5e-7,
// evaluated at z = |x| / sqrt 2 with the 1/2 of Phi = erfc / 2 folded into the coefficients:
//     h = Phi(-|x|);   Phi(x) = x < 0 ? h : 1 - h.
// No cancellation on the negative side (h is computed directly, never as 1 - something), one v_exp_f32, one
// v_rcp_f32, five fmas and three multiplies per element.  Zero maps to zero (t = 1, h = 1/2 to rounding, 0 * Phi); where
// x^2 overflows the exponential's argument is -inf, exp2 gives 0, t is 0 too and h = 0 * 0: no NaN for any finite
// input.  Against float64 (tests/test_gelu_ref_cpu.py, a numpy-fp32 restatement of these lines):
//     |gelu_erf(x) - x Phi(x)| <= 2^-21 |x|,      |gelu_erf_grad(x) - (Phi(x) + x phi(x))| <= 2^-20.
#pragma once
#include "mfma.h"

namespace ec {

constexpr float GELU_P = 0.3275911f * 0.70710678118654752f;         // p / sqrt 2: t = 1 / (1 + GELU_P |x|)
constexpr float GELU_E = -0.5f * 1.4426950408889634f;               // exp(-x^2 / 2) = exp2(GELU_E x^2)
constexpr float GELU_A1 = 0.5f * 0.254829592f, GELU_A2 = 0.5f * -0.284496736f, GELU_A3 = 0.5f * 1.421413741f,
                GELU_A4 = 0.5f * -1.453152027f, GELU_A5 = 0.5f * 1.061405429f;
constexpr float GELU_PHI0 = 0.3989422804014327f;                    // 1 / sqrt(2 pi)

// h = Phi(-|x|) and e = exp(-x^2 / 2)
__device__ __forceinline__ float gelu_tail(float x, float &e)
{
    const float t = __builtin_amdgcn_rcpf(__builtin_fmaf(__builtin_fabsf(x), GELU_P, 1.f));
    e = __builtin_amdgcn_exp2f((x * x) * GELU_E);
    float p = __builtin_fmaf(t, GELU_A5, GELU_A4);
    p = __builtin_fmaf(t, p, GELU_A3);
    p = __builtin_fmaf(t, p, GELU_A2);
    p = __builtin_fmaf(t, p, GELU_A1);
    return (p * t) * e;
}
__device__ __forceinline__ float gelu_erf(float x)
{
    float e;
    const float h = gelu_tail(x, e);
    return x * (x < 0.f ? h : 1.f - h);
}
// d GELU / dx = Phi(x) + x phi(x)
__device__ __forceinline__ float gelu_erf_grad(float x)
{
    float e;
    const float h = gelu_tail(x, e);
    return __builtin_fmaf(x * GELU_PHI0, e, x < 0.f ? h : 1.f - h);
}
// four at a time, as quick_gelu4: the multiplies and fmas as packed fp32 operations (two elements per issue; each one
// correctly rounded operation, so the values are those of gelu_erf)
__device__ __forceinline__ f32x4 gelu_erf4(f32x4 x)
{
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    f32x4 y;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const f32x2 v = {x[2 * k], x[2 * k + 1]};
        const f32x2 a = {__builtin_fabsf(v[0]), __builtin_fabsf(v[1])};
        const f32x2 d = __builtin_elementwise_fma(a, f32x2{GELU_P, GELU_P}, f32x2{1.f, 1.f});
        const f32x2 t = {__builtin_amdgcn_rcpf(d[0]), __builtin_amdgcn_rcpf(d[1])};
        const f32x2 s = (v * v) * GELU_E;
        const f32x2 e = {__builtin_amdgcn_exp2f(s[0]), __builtin_amdgcn_exp2f(s[1])};
        f32x2 p = __builtin_elementwise_fma(t, f32x2{GELU_A5, GELU_A5}, f32x2{GELU_A4, GELU_A4});
        p = __builtin_elementwise_fma(t, p, f32x2{GELU_A3, GELU_A3});
        p = __builtin_elementwise_fma(t, p, f32x2{GELU_A2, GELU_A2});
        p = __builtin_elementwise_fma(t, p, f32x2{GELU_A1, GELU_A1});
        const f32x2 h = (p * t) * e;
        const f32x2 c = 1.f - h;
        const f32x2 o = v * f32x2{v[0] < 0.f ? h[0] : c[0], v[1] < 0.f ? h[1] : c[1]};
        y[2 * k] = o[0], y[2 * k + 1] = o[1];
    }
    return y;
}

}  // namespace ec

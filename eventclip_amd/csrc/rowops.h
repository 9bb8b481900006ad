// Device pieces shared by the row kernels (one wave per row, or one element per thread): the 64-lane reductions and
// the lane-resident LayerNorm row.  Not here: mfma.h's xor_sum / xor_max (row-swap reductions over four 16-lane
// rows), the integer reductions of events.hip, the 16- and 32-lane partial butterflies of attention.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace ec {

// xor butterfly over the wave's 64 lanes: every lane ends with the same value, added / compared in the same order
__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

constexpr int LN_MAXV = 8;  // float4 per lane: width <= 2048

// lanes cover the row in float4 units: unit u = i*64 + lane, valid if u*4 < width
__device__ __forceinline__ int units(int width, int lane)
{
    const int total = width / 4;
    return (total - lane + 63) / 64;  // number of i with i*64 + lane < total
}

// normalises the lane-resident row in place: v = (v - mean) * rstd * gamma + beta
__device__ __forceinline__ void ln_row(float4 (&v)[LN_MAXV], int nv, int width, int lane,
                                       const float *gamma, const float *beta, float eps)
{
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXV; i++)
        if (i < nv) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    const float mean = wave_sum(s) / (float)width;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXV; i++)
        if (i < nv) {
            const float a = v[i].x - mean, b = v[i].y - mean, c = v[i].z - mean, d = v[i].w - mean;
            q += (a * a + b * b) + (c * c + d * d);
        }
    const float rstd = 1.f / __builtin_sqrtf(wave_sum(q) / (float)width + eps);
#pragma unroll
    for (int i = 0; i < LN_MAXV; i++)
        if (i < nv) {
            const int c = (i * 64 + lane) * 4;
            const float4 g = *reinterpret_cast<const float4 *>(gamma + c);
            const float4 b = *reinterpret_cast<const float4 *>(beta + c);
            v[i].x = (v[i].x - mean) * rstd * g.x + b.x;
            v[i].y = (v[i].y - mean) * rstd * g.y + b.y;
            v[i].z = (v[i].z - mean) * rstd * g.z + b.z;
            v[i].w = (v[i].w - mean) * rstd * g.w + b.w;
        }
}

}  // namespace ec

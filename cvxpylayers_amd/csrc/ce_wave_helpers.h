// ce_wave_helpers.h -- small device helpers that more than one kernel family uses beside ce_common.h's reductions
#pragma once
#include "ce_common.h"

// a value that is equal in every lane, moved to scalar registers (frees VGPRs in the iteration loop)
__device__ __forceinline__ double uniform_d(double v) {
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v)), hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// FP32 all-reduce inside aligned groups of CH lanes (DPP, same stages as group_reduce)
template <int CH, bool MAX>
__device__ __forceinline__ float group_reduce_f(float v) {
    auto op = [](float a, float b) { return MAX ? fmaxf(a, b) : a + b; };
    auto mov = [](float x, auto ctrl) { constexpr int CTRL = decltype(ctrl)::value; return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true)); };
    if constexpr (CH >= 2) v = op(v, mov(v, std::integral_constant<int, 0xB1>{}));
    if constexpr (CH >= 4) v = op(v, mov(v, std::integral_constant<int, 0x4E>{}));
    if constexpr (CH >= 8) v = op(v, mov(v, std::integral_constant<int, 0x141>{}));
    if constexpr (CH >= 16) v = op(v, mov(v, std::integral_constant<int, 0x140>{}));
    return v;
}

// sqrt(q) and 1/sqrt(q) to ~1 ulp without the fp64 sqrt + divide expansions (~60 VALU ops): hardware seed (v_rsq_f64) and two
// coupled Goldschmidt steps.  q > 0 and finite; callers guard q == 0.
__device__ __forceinline__ void sqrt_rsqrt(double q, double &s, double &rinv) {
    const double y = __builtin_amdgcn_rsq(q);
    double g = q * y, h = 0.5 * y;
    double r = fma(-h, g, 0.5);
    g = fma(g, r, g); h = fma(h, r, h);
    r = fma(-h, g, 0.5);
    g = fma(g, r, g); h = fma(h, r, h);
    s = g; rinv = 2.0 * h;
}

// block_reduce (ce_common.h) for a workgroup of NWV waves
template <int K, int NWV>
__device__ __forceinline__ void block_reduce_n(double (&v)[K], unsigned maxmask, double *red) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; k++) v[k] = ((maxmask >> k) & 1u) ? wave_reduce_dpp<true>(v[k]) : wave_reduce_dpp<false>(v[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) red[wid * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
        double t[NWV];          // the waves' partial results, requested together (the plain chain waited for each of them: NWV LDS round trips in series behind the barrier)
#pragma unroll
        for (int w = 0; w < NWV; w++) t[w] = red[w * K + k];
        double a = t[0];
#pragma unroll
        for (int w = 1; w < NWV; w++) a = ((maxmask >> k) & 1u) ? fmax(a, t[w]) : a + t[w];
        v[k] = a;
    }
    __syncthreads();
}

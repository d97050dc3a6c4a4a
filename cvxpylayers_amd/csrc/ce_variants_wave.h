// ce_variants_wave.h -- the instantiations of k_fwd_wave (ce_forward_wave.h), stated once: the kernel's translation unit (ce_tu_fwd_wave.hip) instantiates and
// launches from this list, ce_lds_fwd_wave.h selects a row and sums its footprint from it.  Plain C++ (no HIP include).
//
//   X(V, NX, MY, WPS)
//     V    row index (ce_wave_variant)
//     NX   compile-time bound of n: the stride of the LDS matrices is NX + 1, the x vectors live in lanes 0 .. n - 1 (n <= NX)
//     MY   compile-time bound of m: one lane per cone row (m <= MY <= 64)
//     WPS  waves per SIMD the kernel is compiled for (__launch_bounds__(64, WPS): at most 512 / WPS VGPRs)
//   First fit: the first row with n <= NX and m <= MY.  One instance per wave; what is resident per CU is min(4 WPS', LDS) with WPS' the waves per SIMD the
//   allocated registers allow (profiles/fwd_wave/metadata.md).
#pragma once

#define CE_WAVE_VARIANTS(X) \
    X(0, 8, 16, 3)          \
    X(1, 16, 32, 3)         \
    X(2, 32, 64, 3)

// ce_variants_jvp_wave_many.h -- the instantiations of k_jvp_wave_many (ce_jvp_wave_many.h), stated once: the kernel's translation unit
// (ce_tu_jvp_wave_many.hip) instantiates and launches from this list, ce_lds_jvp_wave_many.h selects a row and sums its footprint from it.  Plain C++ (no HIP include).
//
//   X(V, NX, MY, KC, WPS)
//     V    row index (ce_jvp_wave_many_variant); the (NX, MY) of row V are those of row V of CE_NEWTON_WAVE_VARIANTS (ce_variants_newton_wave.h): one served class
//     NX   compile-time bound of n: the stride of the LDS matrices is NX + 1, the equality rows and the rows of the reduced Hessian are NX registers per lane
//     MY   compile-time bound of m: one lane per cone row (m <= MY <= 64)
//     KC   tangents of one wave (the chunk): lane n + k, k < KC, is the right-hand side of tangent k, so KC <= 64 - NX; the panels' stride is KC | 1
//     WPS  waves per SIMD the kernel is compiled for (__launch_bounds__(64, WPS): at most 512 / WPS VGPRs)
//   KC is chosen from the LDS footprint (profiles/jvp_wave_many/metadata.md): the four panels cost (2 m + 2 NX) (KC | 1) doubles beside
//   k_newton_wave's carve, exactly k_bwd_wave_many's sum.  Rows 0 and 1: a forward Jacobian's chunk of KC = NX tangents at 5.6 / 20.4 KB.  Row 2: KC = 32 would be
//   77.7 KB (above the 64 KB a launch gets without a function attribute); KC = 16 is 53.1 KB, 3 waves per CU.
#pragma once

#define CE_JVP_WAVE_MANY_VARIANTS(X) \
    X(0, 8, 16, 8, 4)                \
    X(1, 16, 32, 16, 4)              \
    X(2, 32, 64, 16, 2)

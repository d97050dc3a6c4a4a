// ce_variants_bwd_wave_many.h -- the instantiations of k_bwd_wave_many (ce_backward_wave_many.h), stated once: the kernel's translation unit
// (ce_tu_bwd_wave_many.hip) instantiates and launches from this list, ce_lds_bwd_wave_many.h selects a row and sums its footprint from it.  Plain C++ (no HIP include).
//
//   X(V, NX, MY, KC, WPS)
//     V    row index (ce_bwd_wave_many_variant); the (NX, MY) of row V are those of row V of CE_BWD_WAVE_VARIANTS (ce_variants_bwd_wave.h): one served class
//     NX   compile-time bound of n: the stride of the LDS matrices is NX + 1, the equality rows and the rows of the reduced Hessian are NX registers per lane
//     MY   compile-time bound of m: one lane per cone row (m <= MY <= 64)
//     KC   cotangents of one wave (the chunk): lane n + k, k < KC, is the right-hand side of cotangent k, so KC <= 64 - NX; the panels' stride is KC | 1
//     WPS  waves per SIMD the kernel is compiled for (__launch_bounds__(64, WPS): at most 512 / WPS VGPRs)
//   KC is chosen from the LDS footprint (profiles/bwd_wave_many/metadata.md): the four panels cost (2 m + 2 NX) (KC | 1) doubles beside
//   k_bwd_wave's carve.  Row 0: a Jacobian's K = n <= 8 is one chunk at 5.6 KB (WPS 4: at 8 the row spilled to scratch).  Row 1: K = n <= 16 is one chunk at 20.4 KB (8 waves per CU).  Row 2: KC = 32
//   would be 77.7 KB (2 waves per CU, above the 64 KB a launch gets without an attribute); KC = 16 is 53.1 KB, 3 waves per CU, two chunks for K = 32.
#pragma once

#define CE_BWD_WAVE_MANY_VARIANTS(X) \
    X(0, 8, 16, 8, 4)                \
    X(1, 16, 32, 16, 4)              \
    X(2, 32, 64, 16, 2)

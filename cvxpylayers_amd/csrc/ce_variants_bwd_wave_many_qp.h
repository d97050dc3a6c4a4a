// ce_variants_bwd_wave_many_qp.h -- the instantiations of k_bwd_wave_many_qp (ce_backward_wave_many_qp.h), stated once: the kernel's translation unit
// (ce_tu_bwd_wave_many_qp.hip) instantiates and launches from this list, ce_lds_bwd_wave_many_qp.h selects a row and sums its footprint from it.  Plain C++ (no HIP include).
//
//   X(V, NX, MY, KC, WPS)
//     V    row index (ce_bwd_wave_many_qp_variant); the (NX, MY) of row V are those of row V of CE_BWD_WAVE_QP_VARIANTS (ce_variants_bwd_wave_qp.h): one served class
//     NX   compile-time bound of n: the stride of the three LDS matrices (A, R | B_1^-1, P) is NX + 1, the equality rows and the rows of the reduced Hessian are NX
//          registers per lane
//     MY   compile-time bound of m: one lane per cone row (m <= MY <= 64)
//     KC   cotangents of one wave (the chunk): lane n + k, k < KC, is the right-hand side of cotangent k, so KC <= 64 - NX; the panels' stride is KC | 1
//     WPS  waves per SIMD the kernel is compiled for (__launch_bounds__(64, WPS): at most 512 / WPS VGPRs)
//   KC is chosen from the LDS footprint and, for row 2, a measurement (profiles/bwd_wave_many_qp/metadata.md): the four panels cost
//   (2 m + 2 NX) (KC | 1) doubles beside k_bwd_wave_qp's carve.  Row 0: a Jacobian's K = n <= 8 is one chunk at 6.2 KB.  Row 1: K = n <= 16 is one chunk at 22.6 KB
//   (7 waves per CU).  Row 2: KC = 32 would be above the 64 KB a launch gets without an attribute; KC = 16 is 61.6 KB, 2 waves per CU and two chunks for K = 32;
//   KC = 8 is 49.3 KB, 3 waves per CU and four chunks, each repeating the matrix work.  Measured at (32, 64), K = 32, B = 65536: 78.6 ms at KC = 8 against 92.3 ms at
//   KC = 16 (5.07 against 5.82 ms at B = 4096): the third resident wave hides more latency than the two extra factorisations cost -- KC = 8.
#pragma once

#define CE_BWD_WAVE_MANY_QP_VARIANTS(X) \
    X(0, 8, 16, 8, 4)                   \
    X(1, 16, 32, 16, 4)                 \
    X(2, 32, 64, 8, 2)

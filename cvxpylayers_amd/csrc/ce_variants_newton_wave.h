// ce_variants_newton_wave.h -- the instantiations of k_newton_wave (ce_newton_wave.h), stated once: the kernel's translation unit (ce_tu_newton_wave.hip)
// instantiates both modes (forward derivative, refinement step) of every row and launches from this list, ce_lds_newton_wave.h selects a row and sums its footprint
// from it.  Plain C++ (no HIP include).
//
//   X(V, NX, MY, WPS, WPSR)
//     V    row index (ce_newton_wave_variant)
//     NX   compile-time bound of n: the stride of the LDS matrices is NX + 1, the equality rows and the rows of the reduced Hessian are NX registers per lane
//     MY   compile-time bound of m: one lane per cone row (m <= MY <= 64)
//     WPS  waves per SIMD the forward derivative is compiled for (__launch_bounds__(64, WPS): at most 512 / WPS VGPRs)
//     WPSR the same of the refinement step.  It holds x, the record and rho across the elimination: at k_bwd_wave's WPS rows 0 and 1 spilled two and three
//          registers to scratch, so they are compiled for one wave per SIMD fewer (no scratch in any of the six instantiations)
//   The rows, their bounds and WPS are k_bwd_wave's (ce_variants_bwd_wave.h): the served class is one class.  First fit: the first row with n <= NX and
//   m <= MY.  Budget per row and mode: profiles/newton_wave/metadata.md.
#pragma once

#define CE_NEWTON_WAVE_VARIANTS(X) \
    X(0, 8, 16, 8, 7)              \
    X(1, 16, 32, 6, 5)             \
    X(2, 32, 64, 4, 4)

// ce_variants_newton_wave_qp.h -- the instantiations of k_newton_wave_qp (ce_newton_wave_qp.h), stated once: the kernel's translation unit
// (ce_tu_newton_wave_qp.hip) instantiates both modes (forward derivative, refinement step) of every row and launches from this list, ce_lds_newton_wave_qp.h
// selects a row and sums its footprint from it.  Plain C++ (no HIP include).
//
//   X(V, NX, MY, WPS, WPSR)
//     V    row index (ce_newton_wave_qp_variant)
//     NX   compile-time bound of n: the stride of the three LDS matrices (A, R | B_1^-1, P) is NX + 1, the equality rows and the rows of the reduced Hessian are NX
//          registers per lane
//     MY   compile-time bound of m: one lane per cone row (m <= MY <= 64)
//     WPS  waves per SIMD the forward derivative is compiled for (__launch_bounds__(64, WPS): at most 512 / WPS VGPRs)
//     WPSR the same of the refinement step, which holds x, the record and rho across the elimination: chosen per row from the compiled register counts so that
//          no instantiation has scratch (profiles/newton_wave_qp/metadata.md)
//   The rows and their bounds are k_bwd_wave_qp's (ce_variants_bwd_wave_qp.h): the served class is one class.  First fit: the first row with n <= NX and m <= MY.
#pragma once

#define CE_NEWTON_WAVE_QP_VARIANTS(X) \
    X(0, 8, 16, 8, 7)                 \
    X(1, 16, 32, 6, 5)                \
    X(2, 32, 64, 4, 4)

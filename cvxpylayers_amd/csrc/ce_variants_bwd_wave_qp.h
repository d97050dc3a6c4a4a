// ce_variants_bwd_wave_qp.h -- the instantiations of k_bwd_wave_qp (ce_backward_wave_qp.h), stated once: the kernel's translation unit (ce_tu_bwd_wave_qp.hip)
// instantiates and launches from this list, ce_lds_bwd_wave_qp.h selects a row and sums its footprint from it.  Plain C++ (no HIP include).
//
//   X(V, NX, MY, WPS)
//     V    row index (ce_bwd_wave_qp_variant)
//     NX   compile-time bound of n: the stride of the three LDS matrices (A, R | B_1^-1, P) is NX + 1, the equality rows and the rows of the reduced Hessian are NX
//          registers per lane
//     MY   compile-time bound of m: one lane per cone row (m <= MY <= 64)
//     WPS  waves per SIMD the kernel is compiled for (__launch_bounds__(64, WPS): at most 512 / WPS VGPRs)
//   First fit: the first row with n <= NX and m <= MY.  One instance per wave; registers, LDS and resident instances per CU of every row:
//   profiles/bwd_wave_qp/metadata.md.
#pragma once

#define CE_BWD_WAVE_QP_VARIANTS(X) \
    X(0, 8, 16, 8)                 \
    X(1, 16, 32, 6)                \
    X(2, 32, 64, 4)

// ce_variants_fwd_wave_qp.h -- the instantiations of k_fwd_wave_qp (ce_forward_wave_qp.h), stated once: the kernel's translation unit (ce_tu_fwd_wave_qp.hip)
// instantiates and launches from this list, ce_lds_fwd_wave_qp.h selects a row and sums its footprint from it.  Plain C++ (no HIP include).
//
//   X(V, NX, MY, WPS)
//     V    row index (ce_wave_qp_variant)
//     NX   compile-time bound of n: the stride of the three LDS matrices (A-hat, G, P-hat) is NX + 1, the x vectors live in lanes 0 .. n - 1 (n <= NX)
//     MY   compile-time bound of m: one lane per cone row (m <= MY <= 64)
//     WPS  waves per SIMD the kernel is compiled for (__launch_bounds__(64, WPS): at most 512 / WPS VGPRs)
//   First fit: the first row with n <= NX and m <= MY.  One instance per wave; registers, LDS and resident instances per CU of every row:
//   profiles/fwd_wave_qp/metadata.md.
#pragma once

#define CE_FWD_WAVE_QP_VARIANTS(X) \
    X(0, 8, 16, 3)                 \
    X(1, 16, 32, 3)                \
    X(2, 32, 64, 3)

// ce_lds_newton_wave.h -- served class, row selection and LDS footprint of k_newton_wave (ce_newton_wave.h): the forward derivative and the Newton refinement step of
// one instance per wave.  Plain C++ apart from the __host__ __device__ qualifiers (no HIP include): the kernel carves with these numbers, ce_create selects the row
// and sums the footprint with them.  The served class is k_bwd_wave's (bwd_wave_variant, ce_lds_bwd_wave.h) and so is the carve, to the byte: the prologues stage
// what they need beyond it in the R buffer, which idles until the elimination.
#pragma once
#include <cstddef>
#include "ce_variants_newton_wave.h"
#include "ce_lds_bwd_wave.h"

// (NX, MY) of row v
__host__ __device__ inline void newton_wave_bounds(int v, int *nx, int *my) {
    *nx = 0; *my = 0;
#define X(V, NX, MY, WPS, WPSR) if (v == V) { *nx = NX; *my = MY; }
    CE_NEWTON_WAVE_VARIANTS(X)
#undef X
}

// row of CE_NEWTON_WAVE_VARIANTS that serves the template, -1: not served.  Served: bwd_wave_variant's class; first fit over this list's bounds.
__host__ __device__ inline int newton_wave_variant(int n, int m, int z, int l, int nq, const int *q, int ns, int nep, int np, int nnz_p) {
    if (bwd_wave_variant(n, m, z, l, nq, q, ns, nep, np, nnz_p) < 0) return -1;
#define X(V, NX, MY, WPS, WPSR) if (n <= NX && m <= MY) return V;
    CE_NEWTON_WAVE_VARIANTS(X)
#undef X
    return -1;
}

// why newton_wave_variant returned -1 (ce_last_error of ce_jvp_wave / ce_refine_wave)
__host__ __device__ inline const char *newton_wave_refusal(int n, int m, int ns, int nep, int np, int nnz_p) {
    if (nnz_p > 0) return "the template was created with a P structure (the wave Newton kernel serves a linear objective)";
    if (ns > 0) return "the template has a PSD cone (the wave Newton kernel serves zero, nonnegative and second-order cones)";
    if (nep > 0 || np > 0) return "the template has an exponential / power cone (the wave Newton kernel serves zero, nonnegative and second-order cones)";
    if (n > BWD_WAVE_MAX_N) return "n > 32 (the wave Newton kernel keeps one column per lane of half a wave)";
    if (m > BWD_WAVE_MAX_M) return "m > 64 (the wave Newton kernel keeps one cone row per lane)";
    return "the template is not served by the wave Newton kernel";
}

// doubles of the carve at the top of k_newton_wave<NX, MY>: A (m rows of NX + 1; column NX of a weighted row holds -t), R | B_1^-1 (NX rows of NX + 1; column NX
// holds gamma~; before the elimination: b, or the tangent's b entries), two staging vectors of NX and two of MY, and the NX row indices of the equalities
__host__ __device__ inline size_t newton_wave_lds_doubles(int nx, int my, int n, int m) {
    (void)n;
    return (size_t)(m + nx) * (nx + 1) + 2 * (size_t)nx + 2 * (size_t)my + (size_t)(nx + 1) / 2;
}
// bytes of the launch's dynamic LDS for row `variant`; 0: no such row
__host__ __device__ inline size_t newton_wave_lds_bytes(int variant, int n, int m) {
    int nx, my;
    newton_wave_bounds(variant, &nx, &my);
    if (nx == 0 || n < 1 || m < 1 || n > nx || m > my) return 0;
    return 8 * newton_wave_lds_doubles(nx, my, n, m);
}

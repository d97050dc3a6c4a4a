// ce_lds_newton_wave_qp.h -- served class, row selection and LDS footprint of k_newton_wave_qp (ce_newton_wave_qp.h): the forward derivative and the Newton
// refinement step of one QP instance per wave.  Plain C++ apart from the __host__ __device__ qualifiers (no HIP include): the kernel carves with these numbers,
// ce_create selects the row and sums the footprint with them.  The served class is k_bwd_wave_qp's (bwd_wave_qp_variant, ce_lds_bwd_wave_qp.h) and so is the
// carve, to the byte: the prologues stage what they need beyond it (b, the tangent's b entries) in the R buffer, which idles until the elimination, and the
// tangent of P in the buffer P takes afterwards.
#pragma once
#include <cstddef>
#include "ce_variants_newton_wave_qp.h"
#include "ce_lds_bwd_wave_qp.h"

// (NX, MY) of row v
__host__ __device__ inline void newton_wave_qp_bounds(int v, int *nx, int *my) {
    *nx = 0; *my = 0;
#define X(V, NX, MY, WPS, WPSR) if (v == V) { *nx = NX; *my = MY; }
    CE_NEWTON_WAVE_QP_VARIANTS(X)
#undef X
}

// row of CE_NEWTON_WAVE_QP_VARIANTS that serves the template, -1: not served.  Served: bwd_wave_qp_variant's class -- a P structure, zero / nonnegative /
// second-order cones, n <= 32, m <= 64; first fit over this list's bounds.
__host__ __device__ inline int newton_wave_qp_variant(int n, int m, int z, int l, int nq, const int *q, int ns, int nep, int np, int nnz_p) {
    if (bwd_wave_qp_variant(n, m, z, l, nq, q, ns, nep, np, nnz_p) < 0) return -1;
#define X(V, NX, MY, WPS, WPSR) if (n <= NX && m <= MY) return V;
    CE_NEWTON_WAVE_QP_VARIANTS(X)
#undef X
    return -1;
}

// why newton_wave_qp_variant returned -1 (ce_last_error of ce_jvp_qp_wave / ce_refine_qp_wave)
__host__ __device__ inline const char *newton_wave_qp_refusal(int n, int m, int ns, int nep, int np, int nnz_p) {
    if (nnz_p <= 0) return "the template was created without a P structure (the QP wave Newton kernel serves a quadratic objective; a linear one is ce_jvp_wave's / ce_refine_wave's)";
    if (ns > 0) return "the template has a PSD cone (the QP wave Newton kernel serves zero, nonnegative and second-order cones)";
    if (nep > 0 || np > 0) return "the template has an exponential / power cone (the QP wave Newton kernel serves zero, nonnegative and second-order cones)";
    if (n > BWD_WAVE_QP_MAX_N) return "n > 32 (the QP wave Newton kernel keeps one column per lane of half a wave)";
    if (m > BWD_WAVE_QP_MAX_M) return "m > 64 (the QP wave Newton kernel keeps one cone row per lane)";
    return "the template is not served by the QP wave Newton kernel";
}

// doubles of the carve at the top of k_newton_wave_qp<NX, MY>: k_bwd_wave_qp's -- A (m rows of NX + 1), R | B_1^-1 (NX rows of NX + 1; before the elimination: b,
// or the tangent's b entries), P (n rows of NX + 1; before the elimination of the forward derivative: the tangent of P), two staging vectors of NX and two of MY,
// and the NX row indices of the equalities
__host__ __device__ inline size_t newton_wave_qp_lds_doubles(int nx, int my, int n, int m) { return bwd_wave_qp_lds_doubles(nx, my, n, m); }
// bytes of the launch's dynamic LDS for row `variant`; 0: no such row
__host__ __device__ inline size_t newton_wave_qp_lds_bytes(int variant, int n, int m) {
    int nx, my;
    newton_wave_qp_bounds(variant, &nx, &my);
    if (nx == 0 || n < 1 || m < 1 || n > nx || m > my) return 0;
    return 8 * newton_wave_qp_lds_doubles(nx, my, n, m);
}

// ce_lds_bwd_wave_qp.h -- served class, row selection and LDS footprint of k_bwd_wave_qp (ce_backward_wave_qp.h): the adjoint of one QP instance per wave.  Plain
// C++ apart from the __host__ __device__ qualifiers (no HIP include): the kernel carves with these numbers, ce_create selects the row and sums the footprint with them.
#pragma once
#include <cstddef>
#include "ce_variants_bwd_wave_qp.h"

constexpr int BWD_WAVE_QP_MAX_N = 32, BWD_WAVE_QP_MAX_M = 64;      // one lane per cone row, one lane per variable (and one for the right-hand side)

// (NX, MY) of row v
__host__ __device__ inline void bwd_wave_qp_bounds(int v, int *nx, int *my) {
    *nx = 0; *my = 0;
#define X(V, NX, MY, WPS) if (v == V) { *nx = NX; *my = MY; }
    CE_BWD_WAVE_QP_VARIANTS(X)
#undef X
}

// row of CE_BWD_WAVE_QP_VARIANTS that serves the template, -1: not served.  Served: k_fwd_wave_qp's class -- a quadratic objective (a P structure), zero /
// nonnegative / second-order cones of any dimensions, n <= 32, m <= 64; first fit over the rows' bounds.
__host__ __device__ inline int bwd_wave_qp_variant(int n, int m, int z, int l, int nq, const int *q, int ns, int nep, int np, int nnz_p) {
    if (n < 1 || m < 1 || n > BWD_WAVE_QP_MAX_N || m > BWD_WAVE_QP_MAX_M) return -1;
    if (ns > 0 || nep > 0 || np > 0 || nnz_p <= 0) return -1;
    if (z < 0 || l < 0 || nq < 0) return -1;
    long rows = (long)z + l;
    for (int c = 0; c < nq; c++) { if (!q || q[c] < 1) return -1; rows += q[c]; }
    if (rows != m) return -1;
#define X(V, NX, MY, WPS) if (n <= NX && m <= MY) return V;
    CE_BWD_WAVE_QP_VARIANTS(X)
#undef X
    return -1;
}

// why bwd_wave_qp_variant returned -1 (ce_last_error of ce_vjp_qp_wave)
__host__ __device__ inline const char *bwd_wave_qp_refusal(int n, int m, int ns, int nep, int np, int nnz_p) {
    if (nnz_p <= 0) return "the template was created without a P structure (the QP wave adjoint serves a quadratic objective; a linear one is ce_vjp_wave's)";
    if (ns > 0) return "the template has a PSD cone (the QP wave adjoint serves zero, nonnegative and second-order cones)";
    if (nep > 0 || np > 0) return "the template has an exponential / power cone (the QP wave adjoint serves zero, nonnegative and second-order cones)";
    if (n > BWD_WAVE_QP_MAX_N) return "n > 32 (the QP wave adjoint keeps one column per lane of half a wave)";
    if (m > BWD_WAVE_QP_MAX_M) return "m > 64 (the QP wave adjoint keeps one cone row per lane)";
    return "the template is not served by the QP wave adjoint";
}

// doubles of the carve at the top of k_bwd_wave_qp<NX, MY>: k_bwd_wave's -- A (m rows of NX + 1; column NX of a weighted row holds -t), R | B_1^-1 (NX rows of
// NX + 1; column NX holds d~), two staging vectors of NX and two of MY, the NX row indices of the equalities (ints, rounded up to whole doubles) -- plus P (n rows
// of NX + 1; column NX of a free row ends as -(Z^T P x_p)): 8 n (NX + 1) bytes more
__host__ __device__ inline size_t bwd_wave_qp_lds_doubles(int nx, int my, int n, int m) {
    return (size_t)(m + nx + n) * (nx + 1) + 2 * (size_t)nx + 2 * (size_t)my + (size_t)(nx + 1) / 2;
}
// bytes of the launch's dynamic LDS for row `variant`; 0: no such row
__host__ __device__ inline size_t bwd_wave_qp_lds_bytes(int variant, int n, int m) {
    int nx, my;
    bwd_wave_qp_bounds(variant, &nx, &my);
    if (nx == 0 || n < 1 || m < 1 || n > nx || m > my) return 0;
    return 8 * bwd_wave_qp_lds_doubles(nx, my, n, m);
}

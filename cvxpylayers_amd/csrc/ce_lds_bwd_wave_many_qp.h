// ce_lds_bwd_wave_many_qp.h -- served class, row selection, chunk and LDS footprint of k_bwd_wave_many_qp (ce_backward_wave_many_qp.h): K cotangents of one QP
// instance, one wave per chunk of at most KC.  Plain C++ apart from the __host__ __device__ qualifiers (no HIP include): the kernel carves with these numbers,
// ce_create selects the row and sums the footprint with them.  The served class is k_bwd_wave_qp's, stated there once (ce_lds_bwd_wave_qp.h).
#pragma once
#include <cstddef>
#include "ce_lds_bwd_wave_qp.h"
#include "ce_variants_bwd_wave_many_qp.h"

// (NX, MY, KC) of row v
__host__ __device__ inline void bwd_wave_many_qp_bounds(int v, int *nx, int *my, int *kc) {
    *nx = 0; *my = 0; *kc = 0;
#define X(V, NX, MY, KC, WPS) if (v == V) { *nx = NX; *my = MY; *kc = KC; }
    CE_BWD_WAVE_MANY_QP_VARIANTS(X)
#undef X
}

// row of CE_BWD_WAVE_MANY_QP_VARIANTS that serves the template, -1: not served.  Served: exactly what bwd_wave_qp_variant serves; first fit over the rows' bounds.
__host__ __device__ inline int bwd_wave_many_qp_variant(int n, int m, int z, int l, int nq, const int *q, int ns, int nep, int np, int nnz_p) {
    if (bwd_wave_qp_variant(n, m, z, l, nq, q, ns, nep, np, nnz_p) < 0) return -1;
#define X(V, NX, MY, KC, WPS) if (n <= NX && m <= MY) return V;
    CE_BWD_WAVE_MANY_QP_VARIANTS(X)
#undef X
    return -1;
}

// why bwd_wave_many_qp_variant returned -1 (ce_last_error of ce_vjp_qp_many_wave / ce_vjp_qp_many_params_wave): k_bwd_wave_qp's reasons, the class being the same
__host__ __device__ inline const char *bwd_wave_many_qp_refusal(int n, int m, int ns, int nep, int np, int nnz_p) { return bwd_wave_qp_refusal(n, m, ns, nep, np, nnz_p); }

// the chunk of row `variant`: cotangents one wave serves (0: no such row)
__host__ __device__ inline int bwd_wave_many_qp_chunk(int variant) {
    int nx, my, kc;
    bwd_wave_many_qp_bounds(variant, &nx, &my, &kc);
    return kc;
}

// doubles of the carve at the top of k_bwd_wave_many_qp<NX, MY, KC>, in its order: A (m rows of NX + 1), R | B_1^-1 (NX rows of NX + 1), P (n rows of NX + 1;
// column NX of the three matrices is unused here), two staging vectors of NX and two of MY, the NX row indices of the equalities (ints, rounded up to whole
// doubles), and four panels of stride KC | 1 (odd: a walk down a column and one along a row are both conflict-free): D (m rows: d_k = DPi(v) dy_k), T (m rows:
// e_y . d_k of a boundary cone's t-row until the transform, then -t_k of the weighted rows), FX (NX rows: f_k, then Z^T f_k - Z^T P x_p,k in the free rows, then
// x_free,k there) and DT (NX rows: d~_k of the eliminated equality rows)
__host__ __device__ inline size_t bwd_wave_many_qp_lds_doubles(int nx, int my, int kc, int n, int m) {
    return (size_t)m * (nx + 1) + (size_t)nx * (nx + 1) + (size_t)n * (nx + 1) + 2 * (size_t)nx + 2 * (size_t)my + (size_t)(nx + 1) / 2 +
           (2 * (size_t)m + 2 * (size_t)nx) * (size_t)(kc | 1);
}
// bytes of the launch's dynamic LDS for row `variant`; 0: no such row
__host__ __device__ inline size_t bwd_wave_many_qp_lds_bytes(int variant, int n, int m) {
    int nx, my, kc;
    bwd_wave_many_qp_bounds(variant, &nx, &my, &kc);
    if (nx == 0 || n < 1 || m < 1 || n > nx || m > my) return 0;
    return 8 * bwd_wave_many_qp_lds_doubles(nx, my, kc, n, m);
}

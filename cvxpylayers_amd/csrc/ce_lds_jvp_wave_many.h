// ce_lds_jvp_wave_many.h -- served class, row selection, chunk and LDS footprint of k_jvp_wave_many (ce_jvp_wave_many.h): K tangents of one instance, one wave per
// chunk of at most KC.  Plain C++ apart from the __host__ __device__ qualifiers (no HIP include): the kernel carves with these numbers, ce_create selects the row
// and sums the footprint with them.  The served class is k_newton_wave's, stated there once (ce_lds_newton_wave.h).
#pragma once
#include <cstddef>
#include "ce_lds_newton_wave.h"
#include "ce_variants_jvp_wave_many.h"

// (NX, MY, KC) of row v
__host__ __device__ inline void jvp_wave_many_bounds(int v, int *nx, int *my, int *kc) {
    *nx = 0; *my = 0; *kc = 0;
#define X(V, NX, MY, KC, WPS) if (v == V) { *nx = NX; *my = MY; *kc = KC; }
    CE_JVP_WAVE_MANY_VARIANTS(X)
#undef X
}

// row of CE_JVP_WAVE_MANY_VARIANTS that serves the template, -1: not served.  Served: exactly what newton_wave_variant serves; first fit over the rows' bounds.
__host__ __device__ inline int jvp_wave_many_variant(int n, int m, int z, int l, int nq, const int *q, int ns, int nep, int np, int nnz_p) {
    if (newton_wave_variant(n, m, z, l, nq, q, ns, nep, np, nnz_p) < 0) return -1;
#define X(V, NX, MY, KC, WPS) if (n <= NX && m <= MY) return V;
    CE_JVP_WAVE_MANY_VARIANTS(X)
#undef X
    return -1;
}

// the chunk of row `variant`: tangents one wave serves (0: no such row)
__host__ __device__ inline int jvp_wave_many_chunk(int variant) {
    int nx, my, kc;
    jvp_wave_many_bounds(variant, &nx, &my, &kc);
    return kc;
}

// doubles of the carve at the top of k_jvp_wave_many<NX, MY, KC>: k_newton_wave's (A, R | B_1^-1, two staging vectors of NX and two of MY, the equalities' row
// indices; column NX of the two matrices is unused here) and behind it four panels of stride KC | 1 (odd: a walk down a column and one along a row are both
// conflict-free): GY (m rows: g_y,k of the tangent, kept to the epilogue), T (m rows: the weights u_k of a boundary cone's z-rows and gamma_y,k in its t-row until
// the transform, then -t_k of the weighted rows), FX (NX rows: g_x,k, then f_k, then Z^T f_k in the free rows, then x_free,k there) and DT (NX rows: gamma~_k of
// the eliminated equality rows)
__host__ __device__ inline size_t jvp_wave_many_lds_doubles(int nx, int my, int kc, int n, int m) {
    return newton_wave_lds_doubles(nx, my, n, m) + (2 * (size_t)m + 2 * (size_t)nx) * (size_t)(kc | 1);
}
// bytes of the launch's dynamic LDS for row `variant`; 0: no such row
__host__ __device__ inline size_t jvp_wave_many_lds_bytes(int variant, int n, int m) {
    int nx, my, kc;
    jvp_wave_many_bounds(variant, &nx, &my, &kc);
    if (nx == 0 || n < 1 || m < 1 || n > nx || m > my) return 0;
    return 8 * jvp_wave_many_lds_doubles(nx, my, kc, n, m);
}

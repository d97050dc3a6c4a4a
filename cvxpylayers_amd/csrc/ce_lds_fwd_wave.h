// ce_lds_fwd_wave.h -- served class, row selection and LDS footprint of k_fwd_wave (ce_forward_wave.h): one instance per wave.  Plain C++ apart from the
// __host__ __device__ qualifiers (no HIP include): the kernel carves with these numbers, ce_create selects the row and sums the footprint with them.
#pragma once
#include <cstddef>
#include "ce_variants_wave.h"

constexpr int FWD_WAVE_MAX_N = 32, FWD_WAVE_MAX_M = 64;      // one lane per cone row, one lane per variable
constexpr int FWD_WAVE_ROWS =
#define X(V, NX, MY, WPS) +1
    0 CE_WAVE_VARIANTS(X);
#undef X

// (NX, MY) of row v
__host__ __device__ inline void fwd_wave_bounds(int v, int *nx, int *my) {
    *nx = 0; *my = 0;
#define X(V, NX, MY, WPS) if (v == V) { *nx = NX; *my = MY; }
    CE_WAVE_VARIANTS(X)
#undef X
}

// row of CE_WAVE_VARIANTS that serves the template, -1: not served.  Served: a linear objective (no P structure), zero / nonnegative / second-order cones of any
// dimensions, n <= 32, m <= 64; first fit over the rows' bounds.
__host__ __device__ inline int fwd_wave_variant(int n, int m, int z, int l, int nq, const int *q, int ns, int nep, int np, int nnz_p) {
    if (n < 1 || m < 1 || n > FWD_WAVE_MAX_N || m > FWD_WAVE_MAX_M) return -1;
    if (ns > 0 || nep > 0 || np > 0 || nnz_p > 0) return -1;
    if (z < 0 || l < 0 || nq < 0) return -1;
    long rows = (long)z + l;
    for (int c = 0; c < nq; c++) { if (!q || q[c] < 1) return -1; rows += q[c]; }
    if (rows != m) return -1;
#define X(V, NX, MY, WPS) if (n <= NX && m <= MY) return V;
    CE_WAVE_VARIANTS(X)
#undef X
    return -1;
}

// why fwd_wave_variant returned -1 (ce_last_error of ce_solve_wave)
__host__ __device__ inline const char *fwd_wave_refusal(int n, int m, int ns, int nep, int np, int nnz_p) {
    if (nnz_p > 0) return "the template was created with a P structure (the wave kernel serves a linear objective)";
    if (ns > 0) return "the template has a PSD cone (the wave kernel serves zero, nonnegative and second-order cones)";
    if (nep > 0 || np > 0) return "the template has an exponential / power cone (the wave kernel serves zero, nonnegative and second-order cones)";
    if (n > FWD_WAVE_MAX_N) return "n > 32 (the wave kernel keeps one variable per lane of half a wave)";
    if (m > FWD_WAVE_MAX_M) return "m > 64 (the wave kernel keeps one cone row per lane)";
    return "the template is not served by the wave kernel";
}

// doubles of the carve at the top of k_fwd_wave<NX, MY>: A-hat (m rows of NX + 1), G = K^-1 (n rows of NX + 1), two staging vectors of NX and two of MY
__host__ __device__ inline size_t fwd_wave_lds_doubles(int nx, int my, int n, int m) { return (size_t)(m + n) * (nx + 1) + 2 * (size_t)nx + 2 * (size_t)my; }
// bytes of the launch's dynamic LDS for row `variant`; 0: no such row
__host__ __device__ inline size_t fwd_wave_lds_bytes(int variant, int n, int m) {
    int nx, my;
    fwd_wave_bounds(variant, &nx, &my);
    if (nx == 0 || n < 1 || m < 1 || n > nx || m > my) return 0;
    return 8 * fwd_wave_lds_doubles(nx, my, n, m);
}

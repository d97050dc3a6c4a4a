// ce_lds_bwd_generic.h -- footprint of the size-generic adjoint kernel k_backward (ce_backward.h).  Plain C++ apart from the qualifiers.
#pragma once
#include "ce_lds_common.h"

// bytes of k_backward<a_lds, k_lds>'s dynamic LDS: the carve at the top of the kernel, term by term (panel: T.gen_blocked_b, the panels of the blocked elimination)
__host__ __device__ inline size_t bwd_lds_bytes(const DevT &T, bool a_lds, bool k_lds, int nkcap, int ldk, bool panel = false) {
    const int n = T.n, m = T.m, PB = imax(NT, imax(n, m)), nqs = imax(T.nq, 1);
    size_t d = 0;
    if (a_lds) d += (size_t)m * T.lda;
    if (k_lds) d += (size_t)nkcap * ldk;
    d += 5 * (size_t)m + 2 * (size_t)n + 2 * (size_t)nqs * n + 6 * nqs + PB + NW * 8 + bwd_cone_scratch_doubles(T.ns, T.maxs, m, T.nep + T.np, NW);
    if (!k_lds && panel) d += generic_lu_panel_doubles(nkcap);
    const size_t ints = 2 * (size_t)m + 2 * nqs + 2 * (size_t)nkcap + 4;      // (perm + colrow)
    return d * 8 + ints * 4 + 16;
}

// ce_lds_fwd_generic.h -- footprint of the size-generic forward kernel k_forward (ce_forward_generic.h).  Plain C++ apart from the qualifiers.
#pragma once
#include "ce_lds_common.h"

// bytes of k_forward<a_lds, g_lds>'s dynamic LDS: the carve at the top of the kernel, term by term (panel: T.gen_blocked_f, the panels of the blocked inversion)
__host__ __device__ inline size_t fwd_lds_bytes(const DevT &T, bool a_lds, bool g_lds, bool panel = false) {
    const int n = T.n, m = T.m, l = n + m + 1, PB = imax(NT, imax(n, m));
    size_t d = 0;
    if (a_lds) d += (size_t)m * T.lda;
    if (g_lds) d += (size_t)n * T.ldg;
    d += 2 * (size_t)m + 2 * (size_t)n + 5 * (size_t)l + imax(n, m) + 2 * (size_t)PB + NW * 8 + 2 * imax(T.nq, 1) + NW + 2 * (size_t)n;
    d += fwd_cone_scratch_doubles(T.ns, T.maxs, T.nep + T.np) + 1;      // (+ alignment)
    if (!g_lds && panel) d += generic_gj_panel_doubles(n) + 2;
    return d * 8 + 16;
}

// ce_lds_bwd_rt.h -- thread grid and footprint of the register-tiled adjoint k_backward_rt (ce_backward_rt.h).  Plain C++ apart from the qualifiers.
#pragma once
#include "ce_lds_common.h"

constexpr int BG = 16;   // default thread grid is BG x BG
constexpr int BGC = 16;  // column residues (always one DPP row wide)

__host__ __device__ inline int bwd_rt_union_doubles(int n, int m, int nqs, int TI, int TJ, int BGR = 16) {
    int a = 2 * nqs * n, b = 2 * BGR * TI + 2 * BGC * TJ, c = (NT > m ? NT : m) + m;
    int r = a > b ? a : b;
    return r > c ? r : c;
}

// bytes of k_backward_rt<TI, TJ, *, *, BGR>'s dynamic LDS: the carve at the top of the kernel, term by term (lda = n)
__host__ __device__ inline size_t bwd_rt_lds_bytes(const DevT &T, int TI, int TJ, int BGR) {
    const int n = T.n, m = T.m, nqs = imax(T.nq, 1), nwb = BGR * BGC / 64;
    const size_t d = (size_t)m * n + 3 * (size_t)m + 2 * (size_t)n + 6 * nqs + BGR * TI + 5 /* pinfo: two 16-byte records + alignment */ + nwb * 8 +
                     bwd_cone_scratch_doubles(T.ns, T.maxs, m, T.nep + T.np, nwb) + bwd_rt_union_doubles(n, m, nqs, TI, TJ, BGR);
    const size_t ints = 2 * (size_t)m + 2 * nqs + BGC * TJ + BGR * TI + nwb + 1 + 8;
    return d * 8 + ints * 4 + 16;
}

// ce_lds_fwd_rt.h -- k_forward_rt (ce_forward_rt.h): thread count, fixed LDS part and the fit test of a variant's tiles.  Plain C++ apart from the qualifiers.
#pragma once
#include "ce_lds_common.h"

constexpr int NT2 = 512;
constexpr int NW2 = NT2 / 64;
constexpr int RT_NVEC = 14;
constexpr int RT_EXTRA = NW2 * 8 + NW2 + 16;   // red, wpart, scalars

// whether a template fits the tiles of k_forward_rt<CH1, T1, TG, CH2, T2, VP>; then also the leading dimension of A and the bytes of the kernel's dynamic LDS
__host__ __device__ inline bool rt_fits(const DevT &T, int CH1, int T1, int TG, int CH2, int T2, int VP, int *lda_out, size_t *bytes) {
    if (T.n * CH1 > NT2 || T.m * CH2 > NT2 || CH1 * T1 < T.m || CH1 * TG < T.n || CH2 * T2 < T.n) return false;
    const int reach = imax(imax(T.n + T.m + 1, T.n + CH1 * T1), imax(imax(CH2 * T2, CH1 * TG), imax(NT2 / CH1, NT2 / CH2)));
    if (reach > VP) return false;
    int lda = imax((T.n + 3) & ~3, imax(CH2 * T2, CH1 * TG));
    while (lda % 8 != 4) lda += 4;      // conflict-free interleaved row reads (ds_read_b64, groups of CH2 lanes per row)
    *lda_out = lda;
    *bytes = ((size_t)RT_NVEC * VP + RT_EXTRA + (size_t)T.m * lda) * 8;      // (O_A + m * lda of the layout below)
    return true;
}

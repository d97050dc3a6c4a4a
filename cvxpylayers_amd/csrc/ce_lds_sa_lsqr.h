// ce_lds_sa_lsqr.h -- footprint of the one-kernel LSQR adjoint / forward derivative k_sa_lsqr (ce_shared_a.h).  Plain C++ apart from the qualifiers.
#pragma once
#include "ce_lds_common.h"
#include "ce_lds_psd_mfma.h"

// LDS doubles.  nvv: rows in front of the first PSD block (v = y - s is kept for those only; PSD blocks read y - s once, at the start).
// The partial sums of the dense-row products (2 NT doubles) share the PSD scratch matrices when the template has PSD blocks.
// The forward derivative (FWD) runs the same bidiagonalisation on the same vectors: its footprint is this function's with lsmr = 0.
__host__ __device__ inline size_t sa_lsqr_lds_doubles(int n, int m, int nq, int ns, int maxs, int RP, int nvv, int ntri = 0, int lsmr = 0) {
    const int kp = ns > 0 ? psd_mfma_kp(maxs) : 0;
    return (size_t)(RP > 0 ? 2 * RP + (ns > 0 ? 0 : 2 * NT) : 0) + (size_t)(ns > 0 ? (2 * ns + 2) * kp * (kp + 1) + 2 * kp + 8 : 0) + NW * 8 +
           (size_t)(nvv + (nvv & 1)) + 6 * (size_t)m + 4 * (size_t)n + 5 * (size_t)(nq > 0 ? nq : 1) + 16 + 9 * (size_t)ntri + (ntri & 1) + (lsmr ? (size_t)m + n : 0);      // (LSMR: one more vector, h-bar)
}

// ce_lds_sa_fwd.h -- footprint of the shared-A forward kernel k_sa_fwd (ce_shared_a_fwd.h).  Plain C++ apart from the qualifiers.
#pragma once
#include "ce_lds_psd_mfma.h"

// LDS doubles (see the carve in the kernel)
__host__ __device__ inline size_t sa_fwd_cidx_doubles(int n, int m, int nq, int r, int nsing) {
    return 2 * (size_t)m + ((size_t)(n + 1 + (nsing > 0 ? nsing : 1)) + 1) / 2 + ((size_t)(nq + 1 + (r > 0 ? r : 1)) + 1) / 2 + 2;
}
__host__ __device__ inline size_t sa_fwd_lds_doubles(int n, int m, int nq, int ns, int maxs, int RP, int nth, int ntri = 0) {
    const int l = n + m + 1, lp = l + (l & 1), ne = n + (n & 1), me = m + (m & 1);
    const size_t psd = ns > 0 ? (size_t)ns * maxs * psd_refine_pitch(maxs) + psd_refine_scratch_doubles(maxs) : 0;      // V per block + shared scratch (ce_psd_mfma.h)
    return 6 * (size_t)lp + 2 * (size_t)ne + 2 * (size_t)me + 2 * (size_t)RP * (RP + 1) + 5 * (size_t)RP + 2 * (size_t)(nq > 0 ? nq : 1) +
           psd + (psd & 1) + 2 * nth + (nth / 64) * 8 + 32 + (size_t)(ntri + (ntri & 1));
}

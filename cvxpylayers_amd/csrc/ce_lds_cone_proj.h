// ce_lds_cone_proj.h -- what the host and the kernels of the stand-alone cone projection (ce_cone_proj.h; ce_cone_project / ce_cone_dproject) share: the LDS footprint
// of a PSD block, the layout of the derivative state, and which launches a cone set needs.  Plain C++ apart from the qualifiers
// (tests/test_cone_proj_host.py compiles it with g++ -D__host__= -D__device__=).
#pragma once
#include "ce_lds_psd_mfma.h"    // psd_mfma_kp

constexpr int CONE_PROJ_NT = 256;                      // threads per workgroup of every kernel of the family
constexpr int CONE_PROJ_LDS_BYTES = 160 * 1024;        // LDS of a gfx950 compute unit
constexpr int CONE_PROJ_SOC_SMALL = 16;                // second-order cones up to this dimension take a 16-lane row (four per wave), larger ones a wave
constexpr int CONE_PROJ_PSD_MFMA_MAX = 39;             // PSD orders up to this run on the matrix cores (KP = 16 / 32 / 48, as k_ca_psd_mfma), larger ones psd_jacobi and plain-FMA contractions
// LARGEST SUPPORTED PSD ORDER: 82 (cone_proj_psd_lds_doubles(82) = 20466 doubles <= 20480 = 160 KB; order 83 needs 20964)
constexpr int CONE_PROJ_PSD_MAX = 82;

// pitch of the k x k matrices of a block in LDS: zero-padded KP + 1 on the matrix cores (the operand maps of psd_mfma_gemm), k for psd_jacobi
__host__ __device__ inline int cone_proj_psd_pitch(int k) { return k <= CONE_PROJ_PSD_MFMA_MAX ? psd_mfma_kp(k) + 1 : k; }
__host__ __device__ inline int cone_proj_psd_rows(int k) { return k <= CONE_PROJ_PSD_MFMA_MAX ? psd_mfma_kp(k) : k; }
// LDS doubles of one workgroup of k_cone_psd / k_cone_dpsd at order k: three matrices (S | H, V, T), the rotation parameters (2 rows + 16), the eigenvalues
// (rows) and the reduction scratch (32).  Never below the footprint of the largest matrix-core order, so that it is monotone in k.
__host__ __device__ inline int cone_proj_psd_lds_doubles(int k) {
    const int R = cone_proj_psd_rows(k), P = cone_proj_psd_pitch(k);
    const int own = 3 * R * P + 3 * R + 16 + 32;
    if (k <= CONE_PROJ_PSD_MFMA_MAX) return own;
    const int RM = psd_mfma_kp(CONE_PROJ_PSD_MFMA_MAX), top = 3 * RM * (RM + 1) + 3 * RM + 16 + 32;
    return own > top ? own : top;
}
__host__ __device__ inline bool cone_proj_psd_fits(int k) { return k >= 1 && (long long)cone_proj_psd_lds_doubles(k) * 8 <= CONE_PROJ_LDS_BYTES; }

// doubles of derivative state: eigenvectors (k x k, row-major, columns = eigenvectors) then the k unclipped eigenvalues of a PSD block; the 3 x 3 Jacobian
// (row-major) of a triple.  Zero / nonnegative / second-order cones keep none: their derivative is re-derived from v.
__host__ __device__ inline long long cone_proj_psd_state(int k) { return (long long)k * k + k; }
constexpr int CONE_PROJ_TRIPLE_STATE = 9;

// The layout of a cone set (rows in the solver's order z, l, q, s, ep, p): counts, state sizes and the launches it needs.  Filled by cone_proj_layout() from the
// cone dimensions together with the offset arrays, which the caller owns.
struct ConeProjLayout {
    int z, l, nq, ns, nep, np;
    int m;                    // rows
    int e_row0;               // first row of the triples
    int nq_small, nq_large;   // second-order cones of dimension <= / > CONE_PROJ_SOC_SMALL
    int maxs;                 // largest PSD order (0: none)
    long long state_len;      // doubles of state per instance
    long long tri_state0;     // state offset of the first triple
    // launches: 1 when the kind is present
    int launch_rows, launch_psd, launch_triples;
};

// qoff [nq + 1], soff [ns + 1] (rows, relative to the set's first row), sstate [ns] (state offsets of the PSD blocks), small [nq], large [nq] (cone indices):
// written when non-null.  Returns 0, or the index + 1 of the first PSD order that does not fit LDS (nothing else is then meaningful).
__host__ inline int cone_proj_layout(int z, int l, int nq, const int *q, int ns, const int *s, int nep, int np, ConeProjLayout *L,
                                     int *qoff, int *soff, long long *sstate, int *small, int *large) {
    L->z = z; L->l = l; L->nq = nq; L->ns = ns; L->nep = nep; L->np = np;
    int row = z + l;
    L->nq_small = 0; L->nq_large = 0;
    for (int c = 0; c < nq; c++) {
        if (qoff) qoff[c] = row;
        if (q[c] <= CONE_PROJ_SOC_SMALL) { if (small) small[L->nq_small] = c; L->nq_small++; }
        else { if (large) large[L->nq_large] = c; L->nq_large++; }
        row += q[c];
    }
    if (qoff) qoff[nq] = row;
    L->maxs = 0;
    long long st = 0;
    for (int c = 0; c < ns; c++) {
        if (!cone_proj_psd_fits(s[c])) return c + 1;
        if (soff) soff[c] = row;
        if (sstate) sstate[c] = st;
        st += cone_proj_psd_state(s[c]);
        row += s[c] * (s[c] + 1) / 2;
        if (s[c] > L->maxs) L->maxs = s[c];
    }
    if (soff) soff[ns] = row;
    L->e_row0 = row; L->tri_state0 = st;
    L->state_len = st + (long long)CONE_PROJ_TRIPLE_STATE * (nep + np);
    L->m = row + 3 * (nep + np);
    L->launch_rows = (z + l + nq) > 0; L->launch_psd = ns > 0; L->launch_triples = (nep + np) > 0;
    return 0;
}

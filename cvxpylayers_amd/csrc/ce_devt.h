// ce_devt.h -- the template description the kernels take by value and the launch plan reads (ce_plan.h).  Plain C++: no HIP include.
#pragma once

struct DevT {
    int n, m, nnz_aug, nnzA, z, l, nq, lda, ldg, maxq;
    const int *rowidx;    // [nnz_aug] row of structural entry k
    const int *colidx;    // [nnz_aug] column (n == the b column)
    const int *rowcone;   // [m] -1 for zero / nonneg rows, else SOC index
    const int *qoff;      // [nq+1] first row of SOC c
    int ns, maxs;         // PSD cones, largest order
    const int *soff;      // [ns+1] first row of PSD cone c (svec blocks follow the SOCs, SCS row order z,l,q,s)
    const int *sord;      // [ns] order k of PSD cone c
    int nep, eoff;        // exponential cones (3 rows each) and their first row (after the PSD blocks: SCS row order z,l,q,s,ep,p)
    int np;               // 3-d power cones, after the exponential cones
    const double *pw;     // [np] exponent a of x^a y^(1-a) >= |z|; a < 0: the dual cone of exponent |a| (SCS convention)
    int f2_neumann;       // k_fwd2: a rescale updates G by a Neumann series instead of refactoring (CE_F2_NEUMANN=0 disables)
    int gen_blocked_f, gen_blocked_b;   // size-generic kernels with G / K in global memory: LDS holds the panels of the blocked eliminations (else: unblocked)
};

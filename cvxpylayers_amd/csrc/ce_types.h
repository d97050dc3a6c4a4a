// ce_types.h -- types shared by the translation units of libcone_engine.so and the launcher entry points each kernel
// translation unit exports to the host dispatch (cone_engine.hip).  The kernels are split over several .hip files so that
// they compile in parallel and a change to one kernel family rebuilds one object (csrc/Makefile).
#pragma once
#include <hip/hip_runtime.h>

#include "cone_engine.h"
#include "ce_devt.h"


// arguments of one forward launch (all kernels of the forward family take a subset)
struct CeFwdArgs {
    DevT T; ce_settings S;
    const double *Abm; const double *q; long sqk, sqb;
    const int *idx_at, *idx_ar, *idx_b;
    double *x, *y, *s; int *iters, *status; double *resid;
    const double *P; int nnz_p; const int *idx_p;
    const int *row_perm;        // k_fwd2 WL variants: kernel row -> template row (NULL: rows in template order)
    double *gA, *gG;            // global residency workspaces of the size-generic kernel
    int *iters2;                // k_fwd2: second copy of the iteration counts (engine-owned; NULL: not wanted)
    const int *order;           // k_fwd2: workgroup -> instance (NULL: identity); longest-first dispatch from the previous call's iteration counts
    double *aa_ws;              // size-generic kernel: Anderson-acceleration history, [B][4][lp] doubles of global memory (NULL: plain iteration)
};
struct CeBwdArgs {
    DevT T; int nkcap, ldk;
    const double *Abm, *x, *y, *s, *dx, *dy;
    double *dA, *dq; long sdqk, sdqb; int *adj;
    const double *P; int nnz_p; const int *pmap, *prow, *pcol; int p_tri; double *dP;
    double *gA, *gK;
    int retry;                  // k_backward_rt: 1 = recompute only the instances an earlier launch flagged (adj == 2)
    int *nk_max;                // k_backward_rt: device maximum of the systems' order NK over the batch (NULL: not wanted)
    int *fix;                   // fix[0]: counter, fix[1 ...]: instances whose adjoint system the elimination found rank deficient (or too large for the tile), appended
                                // by the kernels for the LSQR re-solve behind them (cone_engine.hip ce_vjp_qp); NULL: not wanted
    int nonfinal;               // k_backward_rt: 1 = first launch of a two-tile plan (an instance this tile does not hold is not listed: the retry launch serves it)
    int dA_factors;             // k_backward_ns, single-cotangent adjoint only: 1 = store r_y[0 .. m) at the head of the instance's dA row instead of the row's nnz_aug entries
                                // (k_expand_dA behind the launch writes the caller's batch-minor dA from the factors: cone_engine.hip ce_vjp_qp); the launcher hands it to NsNoJvp
};

// k_backward_ns<..., FWD = true> (ce_backward_ns.h): what the forward derivative's elimination reads and writes beside CeBwdArgs' A, x, y, s, adj and fix
struct NsJvp {
    const int *csc_ptr;      // [n + 1]  column starts of the A part in the value order (its rows: DevT::rowidx)
    const int *csr_ptr;      // [m + 1]
    const int *csr_col;      // [nnzA]
    const int *csr_src;      // [nnzA]   position of the entry in the value order
    const int *bpos;         // [m]      position of the row's b entry in the value order (-1: structurally zero)
    const double *tA;        // [B][nnz_aug] tangent of the value rows (NULL: zero)
    const double *tq; long stqk, stqb;       // tangent of q_eval, entry j of instance i at j * stqk + i * stqb (NULL: zero)
    double *dx, *dy, *ds;    // [B][n], [B][m], [B][m] (ds may be NULL)
    int *iters;              // [B] <- 0: a directly solved instance took no LSQR iteration (NULL: not wanted)
};
struct NsNoJvp { int dA_factors = 0; };          // (CeBwdArgs::dA_factors, copied by the launcher: the kernel's own arguments are unpacked)
// k_backward_ns<..., MANY = true> (the adjoint of plain cones with a linear objective): K cotangents on one factorisation of the instance (cone_engine.hip
// ce_vjp_many).  CeBwdArgs' dx, dy, dA, dq and adj point at cotangent 0; cotangent k lies the strides below further (elements; syk = 0: one dy for all)
// rec != NULL (ce_vjp_many_params and its QP / TRI / PSD twins; every type derived from this one carries it): the kernel writes NO dA row -- and the QP kind no dP --; it stores the factor record of pair (k, instance) at rec + k * srk +
// instance * rpitch instead -- r_y[0 .. m), r_tau = 0, r_x[0 .. n): rpitch >= m + 1 + n -- from which k_param_grad (ce_param_grad.h) evaluates the entries it needs
struct NsMany {
    int K;
    long sxk, syk, sAk, sqk, sak;
    double *rec = nullptr; long rpitch = 0, srk = 0;
};
// k_backward_ns<..., FWD = true, ..., MANY = true> (plain cones, P or not): K tangents on one factorisation of the instance (cone_engine.hip ce_jvp_many /
// ce_jvp_qp_many).  Tangent k of instance i: its value row at tA + k * stAk + i * stAb, its q_eval row (n + 1 contiguous entries) at tq + k * stqk + i * stqb; a batch
// stride of 0 is one row shared by every instance.  Outputs of tangent k lie sxk (dx) / syk (dy, ds) / sak (status -- CeBwdArgs' adj -- and iters) elements further
struct NsJvpMany {
    const int *csc_ptr, *csr_ptr, *csr_col, *csr_src, *bpos;          // as NsJvp
    int K;
    const double *tA; long stAk, stAb;       // NULL: zero
    const double *tq; long stqk, stqb;       // NULL: zero
    double *dx, *dy, *ds;    // [K][B][n], [K][B][m], [K][B][m] (ds may be NULL)
    long sxk, syk, sak;
    int *iters;              // [K][B] <- 0 (NULL: not wanted)
};
// k_backward_ns<..., FWD = true, REF = true>: one safeguarded Newton step on the KKT residual (cone_engine.hip ce_refine).  The kernel reads the instance's b through
// bpos and c from q, updates x, y, s IN PLACE when the step is kept, and keeps the per-instance record of the call (one launch = one step)
struct NsRefine {
    const int *bpos;         // [m]      position of the row's b entry in the value order (-1: structurally zero)
    const double *q; long sqk, sqb;          // q_eval, entry j of instance i at j * sqk + i * sqb
    double *x, *y, *s;       // [B][n], [B][m], [B][m] in / out
    const int *status;       // [B] forward status (< 0: the instance is skipped); NULL: every instance is refined
    int *rstatus;            // [B] bit field: 1 a step was kept, 2 a step was rejected by the safeguard, 4 flagged by the elimination, 16 skipped
    int *steps;              // [B] steps kept
    double *resid;           // [B][2] rho before the first step, rho of the returned point
    int first;               // 1: first launch of the call (the record is initialised)
};
// k_backward_ns<..., FWD, REF or not, QP = true>: the quadratic objective of the instance beside what the linear-objective kernel takes
struct NsQp {
    const double *P;         // [B][nnz_p] values of P in the template's structure order
    const double *tP;        // [B][nnz_p] their tangent (the forward derivative only; NULL: zero)
    const int *pmap;         // [n][n]     entry of the structure at (i, j), -1: structural zero; a one-triangle structure maps (i, j) and (j, i) to one entry
    int nnz_p;
};
struct NsJvpQp : NsJvp { NsQp Q; };
struct NsRefineQp : NsRefine { NsQp Q; };
struct NsJvpQpMany : NsJvpMany { NsQp Q; long stPk, stPb; };          // Q.tP: tangent k of instance i's P row at Q.tP + k * stPk + i * stPb
// k_backward_ns<..., FWD = false, ..., QP = true, ..., MANY = true>: K cotangents of the adjoint with P on one factorisation (cone_engine.hip ce_vjp_qp_many).  NsMany's
// strides as ce_vjp_many; entry k of the structure lies at (prow[k], pcol[k]) (p_tri: one triangle is stored and an off-diagonal entry stands for both);
// dP [K][B][nnz_p], cotangent k sPk elements further.  Q.tP is unused
struct NsVjpQpMany : NsMany { NsQp Q; const int *prow, *pcol; int p_tri; double *dP; long sPk; };
// k_backward_ns<..., FWD, REF or not, QP = false, TRI = true>: the same arguments (the triples are described by DevT); types of their own select the launcher
struct NsJvpTri : NsJvp {};
struct NsRefineTri : NsRefine {};
// k_backward_ns<..., FWD, REF or not, ..., PSD = true>: the same arguments again (the PSD blocks are described by DevT: ns, maxs, soff, sord); types of their own
// select the launcher (cone_engine.hip ce_jvp_psd, ce_refine_psd)
struct NsJvpPsd : NsJvp {};
struct NsRefinePsd : NsRefine {};
// k_backward_ns<..., FWD = false, ..., TRI = true, MANY = true>: K cotangents of the adjoint with triples on one factorisation (cone_engine.hip ce_vjp_tri_many).
// NsMany's fields and strides; a type of its own selects the launcher
struct NsVjpTriMany : NsMany {};
// k_backward_ns<..., FWD = true, ..., TRI = true, MANY = true>: K tangents of the forward derivative with triples on one factorisation (cone_engine.hip
// ce_jvp_tri_many).  NsJvpMany's fields and strides; a type of its own selects the launcher.  The name does NOT end in "Many" on purpose: the ledger of
// tests/test_gpu_ns_many_edges.py collects the ce_launch_ns overloads whose type matches Ns\w*Many and pins them to the modes that file covers; this mode's edge
// ledger lives in tests/test_gpu_jvp_tri_many_edges.py (tests/test_jvp_tri_many_args.py pins both facts)
struct NsJvpManyTri : NsJvpMany {};
// k_backward_ns<..., MANY = true, PSD = true>, without and with FWD: K cotangents of the adjoint / K tangents of the forward derivative with PSD blocks on one
// factorisation (cone_engine.hip ce_vjp_psd_many, ce_jvp_psd_many).  NsMany's / NsJvpMany's fields and strides (the blocks are described by DevT); types of their own
// select the launchers.  Neither name ends in "Many", for NsJvpManyTri's reason: their edge ledger lives in tests/test_gpu_psd_many_edges.py
// (tests/test_psd_many_args.py pins the names)
struct NsVjpManyPsd : NsMany {};
struct NsJvpManyPsd : NsJvpMany {};
// k_backward_ns<..., TRI = true, ..., PSD = true>: PSD blocks AND exponential / power triples beside the plain cones, in the four modes the kernel has for the mixed
// kind (cone_engine.hip ce_jvp_psd_tri, ce_refine_psd_tri, ce_vjp_psd_tri_many, ce_jvp_psd_tri_many).  The arguments of the PSD siblings (both cone kinds are
// described by DevT); types of their own select the launchers.  The two many-modes' names do not end in "Many", for NsJvpManyTri's reason: their edge ledger
// lives in tests/test_gpu_psd_tri_edges.py
struct NsJvpPsdTri : NsJvp {};
struct NsRefinePsdTri : NsRefine {};
struct NsVjpManyPsdTri : NsMany {};
struct NsJvpManyPsdTri : NsJvpMany {};

// ---- shared-A kernels (ce_shared_a_fwd.h, ce_shared_a.h, ce_shared_a_ops.h): what the host hands their launchers ----
// fields the product routines read (SaFwd and SaSplit both carry them):
//   r, AdT, drow[r], srow_col[m] (-1: not a singleton row), srow_val[m], scol_ptr[n + 1], scol_row[]
struct SaSplit {
    int r, RP;
    const double *AdT;
    const int *drow, *srow_col;
    const double *srow_val;
    const int *scol_ptr, *scol_row;
    const int *rowslot;          // [m] slot a of a dense row, -1 otherwise
    const int *sing_i;           // [n] the singleton row of column j when it has exactly one (the rule: bounds, -I embeddings), -1: none, -2: several (walk scol_ptr / scol_row)
    const double *sing_v;        // [n] its value (filled with srow_val by k_sa_fill_split)
};

struct SaStruct {            // sparse structure of the template's A part (device arrays, built once per engine)
    const int *csc_ptr;      // [n + 1]   column starts in the value order of the boundary (CSC of [A_cvx | b_cvx], first nnzA entries)
    const int *csc_row;      // [nnzA]
    const int *csr_ptr;      // [m + 1]
    const int *csr_col;      // [nnzA]
    const int *csr_src;      // [nnzA]    position of the entry in the value order
    int nnzA;
    const int *bpos;         // [m]       position of the row's b entry in the value order (-1: structurally zero)
};

// FORWARD derivative (k_sa_lsqr<..., FWD = true>; diffcp's D, oracle/cone_oracle.c apply_M): tangents in, solution tangents out.  Null tangent = zero.
struct SaJvp {
    const double *tA; long stAb;             // [B][nnz_aug] tangent of the boundary's value rows (A part read only when the template's A is per instance)
    const double *tq; long stqk, stqb;       // tangent of q_eval, entry j of instance i at j * stqk + i * stqb (the last entry is ignored)
    double *dx, *dy, *ds;                    // [B][n], [B][m], [B][m] (ds may be null)
};

// k_sa_lsqr walking a re-solve list for K right-hand sides in ONE launch (the many-modes: ce_vjp_many, ce_vjp_tri_many, ce_jvp_many, ce_jvp_tri_many): the walk covers
// K * sel[0] pairs, pair li being right-hand side k = li / sel[0] of instance sel[1 + li % sel[0]]; every per-right-hand-side pointer lies k times its stride (elements)
// further.  K == 1 (the default): today's walk and addressing.  Without a list K is ignored.
struct SaWalkMany {
    int K = 1;
    long sxk = 0, syk = 0, sAk = 0, sqk = 0;     // adjoint: dx, dy (0: one dy for all), dA, dq
    long stAk = 0, stqk = 0, sok = 0, sosk = 0;  // forward: tA, tq, dx (sok), dy and ds (sosk)
    long sak = 0;                                // both: adj_status and iters
    double *rec = nullptr; long rpitch = 0, srk = 0;      // adjoint, rec != NULL (ce_vjp_many_params): the factor record (r_y, r_tau, r_x) of NsMany instead of the dA row
};

struct SaFwd {
    int r, RP;                   // dense rows, padded to a multiple of 16
    const double *AdT;           // [n][RP]  equilibrated dense rows, transposed (solver sign), zero padded
    const int *drow;             // [r]      row index of dense row a
    const int *srow_col;         // [m]      column of a singleton row, -1 otherwise
    const double *srow_val;      // [m]      its (equilibrated, solver-sign) value
    const int *scol_ptr;         // [n + 1]  singleton rows of every column
    const int *scol_row;         // [#singleton entries]
    const double *gs;            // [n]      sum over the singleton rows of column j of d0_i a_i^2
    const double *Dv, *Ev;       // [m], [n] equilibration
    unsigned long long *psd_stats;   // debug (CE_PSD_STATS=1): projections / refinement steps / warm Jacobi fall-backs / cold starts, or null
    double *aa_ws;                   // Anderson acceleration history, [B][4][lp] doubles of global memory (x_prev, f_prev, f_save, [w_prev when it does not fit LDS]; read once
                                     // per acceleration_interval iterations), or null: plain iteration
    int aa_w_lds;                    // the input of the last iteration (w_prev: read by the safeguard, written on two of ten iterations) lives in LDS
    int psd_refine;                  // 1: eigen-refinement on the matrix cores (default); 0 (CE_PSD_REFINE=0): warm-started Jacobi sweeps only, restart at check iterations (round 2)
};

// arguments of one k_sa_fwd launch (T, F, S and the arrays in the kernel's order)
struct CeSaFwdArgs {
    DevT T; SaFwd F; ce_settings S;
    const double *b_hat, *c_hat, *sigma, *nrm_b0, *nrm_c0, *warm_x, *warm_y, *warm_s;
    double *x, *y, *s; int *iters, *status; double *resid;
};
// arguments of one k_sa_lsqr launch; the adjoint reads dx, dy and writes dA, dq, the forward derivative (FWD rows) reads and writes through W instead
struct CeSaLsqrArgs {
    DevT T; SaStruct S; SaSplit F;
    const double *A_vals0; long sA_b; int per_inst;
    const double *q; long sqk, sqb;
    const double *x, *y, *s, *dx, *dy;
    double *dA, *dq; long sdqk, sdqb; int *adj, *iters;
    double atol, btol, conlim; int iter_lim;
    const int *sel; int status_or, a_lds; int *sel_reset;      // the re-solve list of ce_vjp / ce_jvp (ce_shared_a.h)
    SaJvp W;
    SaWalkMany M;
};

// ---- optimal value and its envelope-theorem derivatives (ce_value.h): products and sums over the template's structure, no plan ----
// k_value<JVP>: x [B][n], y [B][m]; the structure's row / column of every entry and the b entry of every row (engine-owned), the P structure (caller-owned)
struct CeValueArgs {
    int B, n, m, nnz_aug, nnz_p;
    const int *rowidx, *colidx, *bpos, *prow, *pcol;
    const double *x, *y;
    const double *A; long sAk, sAb; const double *q; long sqk, sqb; const double *P;      // JVP = false: the values (A: the b entries alone are read)
    double *pobj, *dobj;
    const double *tA; long stAb; const double *tq; long stqk, stqb; const double *tP;     // JVP = true: the tangents (each may be null: zero)
    double *tval;
};
// k_value_vjp_rows / k_value_vjp_tile: g [B] upstream cotangent, skip [B] bytes or null; every output may be null (not wanted)
struct CeValueVjpArgs {
    int B, n, m, nnz_aug, nnz_p;
    const int *rowidx, *colidx, *prow, *pcol;
    const double *x, *y, *g; const unsigned char *skip;
    double *dA; long sdAk, sdAb; double *dq; long sdqk, sdqb; double *dP;
};

// ---- LPGD backward (ce_lpgd.h): the perturbed data of one side, and the differenced envelope gradients of two points; no plan ----
// k_lpgd_perturb: x, dx [B][n], dy [B][m] or null; A [B] rows sAb apart, q and q_out under one stride pair; P, P_out [B][nnz_p]; every output but q_out and
// flags may be null (not written)
struct CeLpgdPerturbArgs {
    int B, n, m, nnz_aug, nnz_p;
    const int *rowidx, *colidx, *bpos, *prow, *pcol;
    const double *x, *dx, *dy;
    const double *A; long sAb; const double *q; long sqk, sqb; const double *P;
    double tau, rho;
    double *q_out, *A_out, *P_out; int *flags;
};
// k_lpgd_grad_rows / k_lpgd_grad_tile: the points (xa, ya), (xb, yb), the divisor delta, skip [B] bytes or null; outputs as CeValueVjpArgs
struct CeLpgdGradArgs {
    int B, n, m, nnz_aug, nnz_p;
    const int *rowidx, *colidx, *prow, *pcol;
    const double *xa, *ya, *xb, *yb; double delta; const unsigned char *skip;
    double *dA; long sdAk, sdAb; double *dq; long sdqk, sdqb; double *dP;
};

// ---- the termination test at a given point (ce_check.h): two sparse products over the template's structure, no plan ----
// k_check_solved: x [B][n], y, s [B][m]; CSR of the A part (rptr, rcol, rsrc), its CSC pointers and rows (cptr, rowidx), the b entry of every row (engine-owned),
// the P structure (caller-owned); gr / gc: threads that share a row / a column (powers of two <= 256, fixed by m and n); eligible [B] or null, tested against emask
struct CeCheckArgs {
    int B, n, m, nnz_aug, nnz_p, gr, gc;
    const int *rptr, *rcol, *rsrc, *cptr, *rowidx, *bpos, *prow, *pcol;
    const double *A; long sAk, sAb; const double *q; long sqk, sqb; const double *P;
    const double *x, *y, *s; const int *eligible; int emask;
    double eps_abs, eps_rel;
    unsigned char *solved; int *status, *iters; double *resid;
};

// ---- parameter gradients from the adjoint's factors (ce_param_grad.h): one streaming kernel, no plan row ----
// k_param_grad: the composed transposed parameter maps of a layer (ptr [rows + 1]; code, kidx, val per entry), the point, the pairs' dq rows and factor records
// (mode PG_RECORDS: the records of NsMany::rec; PG_ROWHEAD, K == 1: r_y at the head of row b of the batch-major dA workspace, the whole row where adj[b] & 8)
enum { PG_RECORDS = 0, PG_ROWHEAD = 1 };
struct CeParamGradArgs {
    int n, m, B, K, rows, slab, mode;
    const int *ptr, *code, *kidx; const double *val;
    const double *x, *y;                                   // [B][n], [B][m]
    const double *dq; long sqK, sqk, sqb;                  // entry j of pair (k, b) at k * sqK + j * sqk + b * sqb
    const double *rec; long rpitch, srk;                   // factors of pair (k, b) at k * srk + b * rpitch
    const int *adj;                                        // [K][B] (PG_ROWHEAD reads bit 8; PG_RECORDS does not read it)
    double *g;                                             // [K][B][rows]
};

// launchers (one per kernel object file; `variant` is a row index of the family's list in ce_variants.h): 0 on success, -1 when the variant is not
// instantiated for the launcher's kind
int ce_launch_fwd2_plain(int variant, int B, size_t lds, hipStream_t st, const CeFwdArgs &a);   // zero / nonneg / SOC
int ce_launch_fwd2_psd(int variant, int B, size_t lds, hipStream_t st, const CeFwdArgs &a);     // + PSD / exponential / power cones
int ce_launch_fwd2_qp(int variant, int B, size_t lds, hipStream_t st, const CeFwdArgs &a);      // quadratic objective inside the kernel
int ce_launch_fwd_rt(int variant, int B, size_t lds, hipStream_t st, const CeFwdArgs &a);
int ce_launch_fwd_generic(int mode, int B, size_t lds, hipStream_t st, const CeFwdArgs &a);
// ce_tu_fwd_wave.hip: k_fwd_wave, one instance per wave (row of CE_WAVE_VARIANTS, ce_variants_wave.h); the resident workgroups per CU of a row
int ce_launch_fwd_wave(int variant, int B, size_t lds, hipStream_t st, const CeFwdArgs &a);
hipError_t ce_occupancy_fwd_wave(int variant, size_t lds, int *blocks);
int ce_launch_bwd_rt_plain(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a);
// k_backward_ns (ce_tu_ns.hip: the linear-objective modes in one object, the two with P in another), one launcher per mode, selected by the mode's argument struct:
// search-free null-space adjoint (plain cones); the same elimination for the forward derivative (a.dx, a.dy, a.dA, a.dq unused) and for one Newton refinement
// step (a.T and a.Abm alone are read); the last two with a quadratic objective
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsNoJvp &w);
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsJvp &w);
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsRefine &w);
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsJvpQp &w);
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsRefineQp &w);
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsJvpTri &w);          // (a third object: exponential / power triples)
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsRefineTri &w);
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsMany &w);               // (a fourth object, ce_tu_ns_many.hip: the adjoint for K cotangents)
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsJvpMany &w);            // (ce_tu_ns_jvp_many.hip, one object per kind: the forward
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsJvpQpMany &w);          //  derivative for K tangents, without and with P)
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsVjpQpMany &w);          // (ce_tu_ns_vjp_qp_many.hip: the adjoint with P for K cotangents)
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsVjpTriMany &w);         // (ce_tu_ns_vjp_tri_many.hip: the adjoint with triples for K cotangents)
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsJvpManyTri &w);         // (ce_tu_ns_jvp_tri_many.hip: the forward derivative with triples for K tangents -- the type's name: see its declaration)
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsJvpPsd &w);             // (ce_tu_ns_psd.hip: the forward derivative and the refinement
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsRefinePsd &w);          //  with PSD blocks)
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsVjpManyPsd &w);         // (ce_tu_ns_vjp_psd_many.hip: the adjoint with PSD blocks for K cotangents)
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsJvpManyPsd &w);         // (ce_tu_ns_jvp_psd_many.hip: the forward derivative with PSD blocks for K tangents)
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsJvpPsdTri &w);          // (ce_tu_ns_psd_tri.hip: the forward derivative and the refinement
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsRefinePsdTri &w);       //  with PSD blocks and triples)
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsVjpManyPsdTri &w);      // (ce_tu_ns_vjp_psd_tri_many.hip: the adjoint with both for K cotangents)
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsJvpManyPsdTri &w);      // (ce_tu_ns_jvp_psd_tri_many.hip: the forward derivative with both for K tangents)
int ce_launch_bwd_rt_psd(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a);
int ce_launch_bwd_generic(int mode, int B, size_t lds, hipStream_t st, const CeBwdArgs &a);
int ce_launch_sa_fwd(int variant, int B, size_t lds, hipStream_t st, const CeSaFwdArgs &a);     // row of CE_SA_FWD_VARIANTS (its thread count is the row's)
int ce_launch_sa_lsqr(int variant, int grid, size_t lds, hipStream_t st, const CeSaLsqrArgs &a);      // row of CE_SA_LSQR_VARIANTS; grid: B, or the fixed grid that walks a.sel
// k_sa_fill_split (ce_shared_a_ops.h; its arguments in the kernel's order): refills the split's A_d^T (zeroed by the caller) and singleton values from this call's A
void ce_launch_sa_fill_split(hipStream_t st, int nnzA, int RP, const int *rowidx, const int *colidx, const int *rowslot, const double *vals, double *AdT, double *srow_val,
                             const int *sing_i, double *sing_v);
// ce_tu_value.hip: one workgroup per instance / per VAL_IPB instances / per (64-instance tile, chunk of kchunk entries); the LDS sizes are the host's (value_lds_*)
void ce_launch_value(bool jvp, size_t lds, hipStream_t st, const CeValueArgs &a);
void ce_launch_value_vjp_rows(size_t lds, hipStream_t st, const CeValueVjpArgs &a);
void ce_launch_value_vjp_tile(bool staged, int chunks, int kchunk, int wdq, size_t lds, hipStream_t st, const CeValueVjpArgs &a);
size_t ce_value_lds(int n, int m);               // k_value
size_t ce_value_vjp_rows_lds(int n, int m);      // k_value_vjp_rows
size_t ce_value_vjp_tile_lds(int n, int m);      // k_value_vjp_tile<STAGED = true>
// ce_tu_check.hip: one workgroup per instance, then one workgroup that counts; staged: the instance's value row sits in LDS (lds includes it)
void ce_launch_check_solved(bool staged, size_t lds, hipStream_t st, const CeCheckArgs &a, int *n_unsolved);
size_t ce_check_lds(int n, int m, int nnz_staged);      // k_check_solved: the vectors of one instance + nnz_staged values
// ce_tu_lpgd.hip: one workgroup per VAL_IPB instances (perturb, grad_rows) / per (64-instance tile, chunk of kchunk entries)
void ce_launch_lpgd_perturb(hipStream_t st, const CeLpgdPerturbArgs &a);
void ce_launch_lpgd_grad_rows(size_t lds, hipStream_t st, const CeLpgdGradArgs &a);
void ce_launch_lpgd_grad_tile(bool staged, int chunks, int kchunk, int wdq, size_t lds, hipStream_t st, const CeLpgdGradArgs &a);
size_t ce_lpgd_grad_rows_lds(int n, int m);      // k_lpgd_grad_rows
size_t ce_lpgd_grad_tile_lds(int n, int m);      // k_lpgd_grad_tile<STAGED = true>
// ce_tu_param_grad.hip: tiles of 16, 8, 4 or 2 pairs (the largest whose footprint leaves two workgroups per CU; 2 whenever it fits at all) x slabs of rows; a.slab is
// the launcher's to set.  -1: the factors of two pairs exceed LDS (nothing is launched)
int ce_launch_param_grad(hipStream_t st, const CeParamGradArgs &a);
hipError_t ce_setattr_param_grad(int bytes);
// raise the dynamic-LDS limit of every kernel of the family
hipError_t ce_setattr_fwd2_plain(int bytes);
hipError_t ce_setattr_fwd2_psd(int bytes);
hipError_t ce_setattr_fwd2_qp(int bytes);
hipError_t ce_setattr_fwd_rt(int bytes);
hipError_t ce_setattr_fwd_generic(int bytes);
hipError_t ce_setattr_bwd_rt_plain(int bytes);
hipError_t ce_setattr_bwd_rt_psd(int bytes);
hipError_t ce_setattr_ns(int bytes);
hipError_t ce_setattr_ns_qp(int bytes);
hipError_t ce_setattr_ns_tri(int bytes);
hipError_t ce_setattr_ns_many(int bytes);
hipError_t ce_setattr_ns_jvp_many(int bytes);
hipError_t ce_setattr_ns_jvp_qp_many(int bytes);
hipError_t ce_setattr_ns_vjp_qp_many(int bytes);
hipError_t ce_setattr_ns_vjp_tri_many(int bytes);
hipError_t ce_setattr_ns_jvp_tri_many(int bytes);
hipError_t ce_setattr_ns_psd(int bytes);
hipError_t ce_setattr_ns_vjp_psd_many(int bytes);
hipError_t ce_setattr_ns_jvp_psd_many(int bytes);
hipError_t ce_setattr_ns_psd_tri(int bytes);
hipError_t ce_setattr_ns_vjp_psd_tri_many(int bytes);
hipError_t ce_setattr_ns_jvp_psd_tri_many(int bytes);
hipError_t ce_setattr_bwd_generic(int bytes);
hipError_t ce_setattr_sa_fwd(int bytes);
hipError_t ce_setattr_sa_lsqr(int bytes);
hipError_t ce_setattr_value(int bytes);
hipError_t ce_setattr_lpgd(int bytes);
hipError_t ce_setattr_check(int bytes);

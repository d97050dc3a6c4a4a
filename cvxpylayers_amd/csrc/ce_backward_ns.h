// ce_backward_ns.h -- SEARCH-FREE structured direct adjoint (round 6; hot path of the default adjoint for plain-cone templates).
//
// Same system as ce_backward_rt.h (diffcp's adjoint M^T r = dz with r_tau pinned to 0, reduced cone block by cone block to the saddle system
//        H r_x - B^T mu = f,   B r_x = d_B,        H = sum_c theta_c A_z^T (I - zh zh^T) A_z  (symmetric PSD),   B = the neq equality rows),
// but it is no longer eliminated as ONE (n + neq)-order matrix with a partial-pivoting search per pivot (59 serial pivots x 2.1 k cycles = 128 k of the
// 214 k cycles of an instance of the metric configuration, profiles/r05/z_setup_phase_cycles.log).  Null-space elimination instead:
//   1. B (neq x n, neq ~ 9) is brought to reduced row-echelon form with COLUMN pivoting by ONE wave, in place in LDS (the equality rows are rows of A;
//      a boundary cone's e_y row overwrites the cone's t-row, which H does not need): B P = [I  R],  x_piv = d~ - R x_free.  The only pivot searches left
//      are these neq wave-local ones (DPP butterflies, no workgroup barrier); the multipliers of the elimination stay in the pivot columns (the
//      transposed product B_1^-T g that yields mu is their reverse replay).
//   2. the rows that make up H are transformed to the null-space basis, a~_k = Z^T a_k = a_k[free] - R^T a_k[piv], in place;
//   3. the reduced Hessian Z^T H Z = sum_k w_k a~_k a~_k^T (order nf = n - neq ~ 41, with the right-hand side Z^T (f - H x_p) as one more column) is
//      accumulated on the MATRIX CORES in the accumulator layout of k_fwd2's S formation (half the k-rows and a quarter of the tiles of round 5's H);
//   4. it is symmetric positive definite on a regular instance: solved by k_fwd2's blocked SWEEP on the matrix cores (v_mfma_f64_16x16x4_f64 rank-4
//      updates, diagonal 4 x 4 pivot blocks, one barrier per block of four, NO search): ~11 blocks instead of 59 pivots;
//   5. x_piv, then mu = B_1^-T (H r_x - f)[piv], then r_y and the outputs exactly as ce_backward_rt.h.
// Rank deficiency (a redundant equality row, a reduced Hessian that is singular on the null space: the degenerate active sets of LP-like programs) shows up
// as a vanishing pivot in step 1 or 4: the variable is dropped (pivot inverse 0, finite numbers), the instance is flagged (adj_status bit 2 = 4) and appended to
// the device-side list whose instances the LSQR kernel behind this launch re-solves with diffcp's own method (cone_engine.hip ce_vjp_qp) -- this kernel is only
// launched when that re-solve is armed, so its answer on such instances is never the final one.
//
//
// FWD = true: the FORWARD derivative (diffcp's `derivative`, cone_engine.hip ce_jvp) by the same elimination.  With d_tau pinned to 0 (M z = 0 at a solution and the
// outputs do not change under d <- d + alpha z) diffcp's M d = -g, g = dQ pi, leaves  A^T D d_y = -g_x,  -A d_x + (I - D) d_y = -g_y  (A in the solver form stored
// here): the transpose of the adjoint's block.  In the eigenbasis of D per cone (eta = W^T d_y, gamma = W^T g_y, rotated rows a~): lambda = 1 rows are the
// equalities  a~ d_x = gamma  with eta their multiplier, lambda = 0 rows give  eta = a~ d_x - gamma,  the others  eta = (a~ d_x - gamma) / (1 - lambda), so
//        H d_x + B^T eta_B = -g_x + sum theta a~^T gamma,      B d_x = gamma_B
// with the H and B above:  f = -g_x + sum theta a~^T gamma,  d_B = gamma_B,  eta_B = -mu.  Load, classification, numbering, a_z, the e_y rows, the weighted-row list
// and steps 1-4 are stated once; FWD has its own PROLOGUE (g from the instance's tangent row through the template's CSC / CSR structure and bpos, tangents in the
// boundary convention of k_sa_lsqr<FWD>; gamma_y, gamma_s and the weights of f per boundary cone in the classification pass) and its own EPILOGUE behind mu
// (eta for every row, rotated back:  dx = d_x,  dy = W lambda eta,  ds = -W (1 - lambda) eta).  It uses the adjoint's LDS buffers (y and x wait in tvec and rx for the
// tangent products; g_y lives in dv, g_x in fvec): the footprint is bwd_ns_lds_bytes_of, the plan's ns_lds serves both.  Flags and the re-solve list as the adjoint.
//
// REF = true (with FWD): one safeguarded NEWTON STEP on the KKT residual (cone_engine.hip ce_refine).  With v = y - s, y^ = Pi(v), s^ = y^ - v the residual map
//        F_x = A^T y^ + c,   F_y = A x + s^ - b        has the Jacobian system   A^T D dv = -F_x,  -A dx + (I - D) dv = F_y,
// the forward derivative's block with g_x = F_x, g_y = -F_y: the FWD path runs unchanged between another PROLOGUE (projection, the two dense products with the A
// in LDS, b through bpos, c from q_eval, rho before) and another EPILOGUE behind eta (x+ = x + dx, v+ = v + dy - ds, projection, the value row scattered into LDS
// again, rho after, keep or reject, x, y, s written in place).  No buffer beyond the adjoint's (the block maxima go through `red`).  A flagged instance keeps its point.
//
// QP = true (with FWD, REF or not): a quadratic objective 1/2 x^T P x inside the elimination (cone_engine.hip ce_jvp_qp, ce_refine_qp).  The stationarity row gains
// P:  P d_x + A^T D d_v = -g_x  with  g_x = tP x + tA^T y + tc  (REF: F_x = P x + A^T y^ + c), so the saddle system is  (H + P) d_x + B^T eta_B = f,  B d_x = gamma_B
// with the f above.  P (dense, symmetric, n x n, behind the index arrays in LDS: bwd_ns_qp_lds_bytes_of) enters in three places, everything else is shared:
//   - its rows go through the null-space transform of step 2 like weighted rows (p~_j = Z^T p_j in place, t_j = p_j . x_p), and
//     Z^T P Z = sum_j z_j p~_j^T  (z_j = row j of Z: a unit vector for a free column, -R[e,:] for the pivot column of equality e) is one more run of
//     v_mfma_f64_16x16x4_f64 accumulations into the tiles of step 3, with  sum_j z_j t_j = Z^T P x_p  in the right-hand-side column;
//   - g = ((H + P) r_x - f)[piv] for the multipliers: the pivot COLUMNS of P are untouched by the transform and P is symmetric.
// With no active row at all H = 0 and the reduced Hessian is P alone: regular when P is positive definite, where the linear objective flags the instance.
// A flagged instance keeps the dropped-variable answer with status 4 (no LSQR has a P term, so no re-solve list exists behind a QP launch).
//
// TRI = true (with FWD, REF or not, never QP): exponential and 3-d power triples beside the plain cones.  D Pi_K*(v) of a triple is W diag(lambda) W^T (ce_expcone.h
// exp_dual_eig / pow_dual_eig, one thread per triple in the classification pass; lambda snapped to 0 / 1 within 1e-9 as k_backward_rt does, so both kernels decide
// alike).  The triple's three rows of A are rotated in place, A_c <- W^T A_c, and gamma = W^T g_y with them: afterwards a rotated row is an ordinary equality
// (lambda = 1, numbered with the others), a dropped row (lambda = 0, nothing in H) or ONE weighted row of the list (weight theta = lambda / (1 - lambda), theta gamma a~
// in f), and steps 1-5 run unchanged.  The epilogue computes eta for the three rotated rows and rotates back,  dy = W lambda eta,  ds = -W (1 - lambda) eta.
// REF: y-hat of a triple is exp_project_dual / pow_project_dual_of_entry from the cold start exp_dual_eig / pow_dual_eig evaluate at -- the same decision, the
// rule of ns_soc_kind.  W and lambda live behind the index arrays in LDS (ns_layout's TRI mode).
//
// PSD = true (with FWD, REF or not, or with MANY, FWD or not -- below; never QP; with TRI: the last paragraph of this list): PSD blocks beside the plain cones (cone_engine.hip ce_jvp_psd, ce_refine_psd: entry points of their own, ce_jvp
// and ce_refine keep refusing such templates).  smat(v_c) = U Lambda U^T by the workgroup's Jacobi sweeps (ce_psd_jacobi.h); in the basis E_ab = svec(sym(u_a u_b^T))
// D Pi is diagonal with eigenvalue B_ab (1 / 0 / l+ / (l+ - l-), k_backward_rt's comparisons, no snap).  The block's rows of A are rotated in place,
// a~ = svec(U^T smat(a) U) per column, gamma = Q^T g_y with them; afterwards a rotated row is an equality, a dropped row or ONE weighted row of the list, exactly a
// triple's rows, and steps 1-5 run unchanged.  The epilogue computes eta of the rotated rows and rotates back,  dy_c = Q (B o eta),  ds_c = -Q ((1 - B) o eta),
// Q r = svec(U smat(r) U^T).  REF: y-hat_c = svec(U max(Lambda, 0) U^T) from the decomposition that gives B; a full step that fails the safeguard is tried again at
// 1/2, 1/4, 1/8 of its length (the REF epilogue: this mode alone).  NS_TRI_STIFF flags the forward derivative's instance
// with a weighted PSD row of 1 - B below it: carried over, not measured on PSD rows.  U, Lambda, B and the scratch live behind the index arrays (ns_layout's PSD mode).
//
// MANY = true: K right-hand sides on ONE factorisation of the instance.  Steps 1-4 depend on (A, x, y, s [, P]) alone and run once, on a zero right-hand side; the sweep is an
// in-place inversion, so -(Z^T (H [+ P]) Z)^-1 stays in the accumulator tiles and B_1^-1 in the pivot columns, and each right-hand side is rebuilt behind the sweep, then
// step 5 and the mode's epilogue run on the same buffers.  Without FWD (cone_engine.hip ce_vjp_many): K cotangents of the plain adjoint.  With FWD, QP or not
// (ce_jvp_many, ce_jvp_qp_many): K tangents -- per tangent the forward PROLOGUE again (x and y re-read from global memory: the tangent products need the tangent's values
// and the point, not A, which is transformed by now; a tangent's row lies at k * stride_k + inst * stride_b, stride_b == 0 being one row for the whole batch), gamma and
// the weights of f from the retained classification, d~ from the in-place inverse, t_q for the list rows (QP: Z^T P x_p from the transformed rows of P, whose pivot
// columns are untouched), f with the treatment of the two rows that are gone (a_z, and the t-row a_y overwrote), x_free from the tiles, step 5 and the forward EPILOGUE
// unchanged.  Rank deficiency belongs to the matrix: the instance is flagged for every k and listed once.  REF never comes with MANY.
// With FWD and TRI (cone_engine.hip ce_jvp_tri_many): K tangents with exponential / power triples.  Once per instance the TRI code above runs as it stands on a zero
// right-hand side (exp_dual_eig / pow_dual_eig once per triple, the snap, A_c <- W^T A_c, the numbering); W, lambda, rkind, eqrow and the list entries stay in LDS.
// Per tangent the plain many-tangent rebuild plus, per triple, gamma_c = W^T g_y,c: a lambda = 1 row puts its gamma into d_B, a lambda = 0 row contributes nothing, a
// weighted row puts theta gamma into its weight slot (qv2, by row) and theta t into its list entry; step 5 and the TRI forward epilogue follow unchanged.
// NS_TRI_STIFF flags the instance for every k like a vanishing pivot, the forward derivative's own rule.  The footprint is the triples' (tri_ns_variant, tri_ns_lds).
// Without FWD, with TRI (cone_engine.hip ce_vjp_tri_many): K cotangents of the adjoint with exponential / power triples, the one adjoint with triples this kernel has.
// Once per instance the TRI code above runs as it stands (exp_dual_eig / pow_dual_eig once per triple, A_c <- W^T A_c, the weighted rows numbered behind the
// boundary cones'), W, lambda, rkind and eqrow stay in LDS, and steps 1-4 run on a zero right-hand side on the triples' footprint (tri_ns_variant, tri_ns_lds).  Per
// cotangent the plain rebuild plus, per triple, h = W^T dy_c: a lambda = 1 row gives its entry of d_B, a lambda = 0 row d = 0, a weighted row d = lambda h and the
// share u = theta h of f = dx + A^T u on the rotated row (the transpose of the forward's theta gamma a~; k_backward_rt's a~ d / (1 - lambda)); behind step 5
// r~_y = mu (lambda = 1), 0 (lambda = 0), (d - lambda a~ . r_x) / (1 - lambda) (weighted), rotated back r_y,c = W r~_y,c in front of the output pass.  NS_TRI_STIFF
// below flags the instance for every k like a vanishing pivot: the threshold is the forward derivative's measured law, carried over, not measured for the adjoint.
// Without FWD, with QP (cone_engine.hip ce_vjp_qp_many): K cotangents of the adjoint with P.  The system is (H + P) r_x - B^T mu = f, B r_x = d_B; per cotangent the plain
// many-cotangent rebuild plus the P terms of the many-tangent one (t_j = p_j . x_p and Z^T P x_p in the reduced right-hand side, (P r_x)[piv] in g), and one more output
// row dP = -sym(r_x x^T) through the structure.  No re-solve list: a flagged instance keeps the dropped-variable answer, status 4 for every k.
// With PSD, FWD or not (cone_engine.hip ce_jvp_psd_many, ce_vjp_psd_many; never REF, QP or TRI beside them): K tangents / K cotangents with PSD blocks, the two modes
// that make seventeen.  Once per instance the PSD code above runs as it stands on a zero right-hand side (psd_decompose, A_c rotated in place column by column, B -> lamp,
// the weighted rows numbered behind the boundary cones', NS_TRI_STIFF); psdU, psdEv, lamp, rkind and eqrow stay in LDS behind the sweep on the blocks' footprint
// (psd_ns_variant, psd_ns_lds: no segment is added -- psdScr idles behind the decomposition, the first (X, W) pair of psdXW is the rotation workspace of a right-hand
// side: psd_rotate_vec, all threads, three phases per block behind workgroup-uniform barriers).  Per tangent the plain many-tangent rebuild plus gamma_c = Q^T g_y,c per
// block: a B = 1 row puts its gamma into d_B, a B = 0 row contributes nothing, a weighted row puts theta gamma into its weight slot (qv2, by row) and theta t into its
// list entry, as a triple's; step 5 and the PSD forward epilogue follow unchanged.  Per cotangent the plain many-cotangent rebuild plus h = Q^T dy_c per block: a B = 1
// row gives its entry of d_B, a B = 0 row d = 0, a weighted row d = B h and the share u = theta h of f = dx + A^T u on the rotated row; behind step 5
// r~_y = mu (B = 1), 0 (B = 0), (d - B a~ . r_x) / (1 - B) (weighted), rotated back r_y,c = Q r~_y,c in front of the unchanged output pass (original basis, ce_vjp's
// boundary convention).  It is the one adjoint with PSD blocks this kernel has.  Flags belong to the matrix: a vanishing pivot, neq > n or a weighted PSD row with
// 1 - B < NS_TRI_STIFF flag the instance for every k and it is listed once -- the threshold is carried over AGAIN (the triples' forward law -> the triples' adjoint ->
// PSD rows, in both directions): not measured on PSD rows, not measured for an adjoint.  A flagged instance runs to the same barriers as any other.
// TRI and PSD together (never QP; FWD, FWD + REF, MANY, FWD + MANY -- cone_engine.hip ce_jvp_psd_tri, ce_refine_psd_tri, ce_vjp_psd_tri_many, ce_jvp_psd_tri_many; a
// single-cotangent adjoint stays k_backward_rt's): a template with PSD blocks AND triples (log_det: one block beside one exponential cone per diagonal entry).  The rows
// are z, l, q, then the blocks' (psd0 .. T.eoff - 1), then the triples' (T.eoff .. m - 1), and every phase of either kind above is a branch of its own on its own rows:
// the mixed kind runs both, in sequence -- each triple's D Pi diagonalised, snapped, its rows rotated; each block decomposed and its rows rotated; both kinds' weighted
// rows numbered behind the boundary cones' (the triples' first, then the blocks': each pass reads misc[3] behind the other's barrier; at most m entries together);
// steps 1-4; both epilogues and both rotations back.  MANY: per right-hand side both gamma_c = W^T g per triple and gamma = Q^T g per block.  REF: y-hat of a triple
// from its cold-start decision and y-hat of a block from its decomposition inside one acceptance test, with the PSD kind's shortened steps.  NS_TRI_STIFF flags from
// either kind's weighted rows (carried over once more).  The segments are ns_layout's with both counts: Wt, lamt, then psdU .. psdXW (psd_tri_ns_variant, psd_tri_ns_lds).
//
// Plain cones (zero / nonnegative / second-order), with TRI exponential / power triples in the forward modes (one tangent or many) and in the many-cotangent adjoint.  PSD blocks in the forward
// derivative, the refinement, and the two many-modes with PSD.  The SINGLE-cotangent adjoint of PSD templates keeps k_backward_rt, and so do the single-cotangent adjoint
// with triples and the single-cotangent adjoint with a quadratic objective.
#pragma once
#include "ce_common.h"
#include "ce_expcone.h"            // TRI: exp_dual_eig, pow_dual_eig, exp_project_dual, pow_project_dual_of_entry
#include "ce_psd_jacobi.h"         // PSD: psd_jacobi
#include "ce_dA_entry.h"           // ce_dA_entry: the entry of the dA row, shared with k_expand_dA

#include "ce_ns_layout.h"          // ns_layout: the LDS segments of this kernel and its footprint (what the launch plan and tests/test_ns_layout_host.py use); bwd_ns_ldp, bwd_ns_nsl,
                                   // bwd_ns_kwmax, bwd_ns_union_doubles.  The carve below is still the kernel's own statement of the same layout.

#ifdef CE_TIMING
#define NS_STAMP(i) do { __syncthreads(); if (threadIdx.x == 0) tstamp[i] = __builtin_readcyclecounter(); } while (0)
#define NS_SUB(i) do { if (threadIdx.x == 0) tsub[i] = __builtin_readcyclecounter(); } while (0)          // thread 0's clock, no barrier
#else
#define NS_STAMP(i) do { } while (0)
#define NS_SUB(i) do { } while (0)
#endif

// where v = (t0, z) of a second-order cone of dimension d, |z| = nz, lies: 0 inside the cone (DPi = I), 1 inside its polar (DPi = 0), 2 outside both (lam: the
// eigenvalue (t0 + nz) / (2 nz) of DPi on z-hat's complement).  ONE statement for the classification pass and for the projection of the refinement mode: the Newton
// step is right only when D and y-hat = Pi(v) come from the same decision.
__device__ __forceinline__ int ns_soc_kind(int d, double t0, double nz, double &lam) {
    int kind; lam = 0.0;
    if (d == 1) kind = t0 >= 0 ? 0 : 1;
    else if (nz <= t0) kind = 0; else if (nz <= -t0) kind = 1; else { kind = 2; lam = (t0 + nz) / (2 * nz); }
    return kind;
}

// TRI: the forward derivative hands an instance with a weighted triple row of 1 - lambda below this to the re-solve (the elimination's error at the threshold, by the
// measured law: 0.03 eps / NS_TRI_STIFF^2 = 3e-8).  The many-cotangent adjoint with triples carries the rule over as it stands (flagged for every k): the law was
// measured on the forward derivative, not on the adjoint.  PSD rows carry it over again, in the forward modes and in the many-cotangent adjoint: not measured there.
constexpr double NS_TRI_STIFF = 1e-5;

template <bool FWD, bool REF = false, bool QP = false, bool TRI = false, bool MANY = false, bool PSD = false> struct NsFwdArg { typedef NsNoJvp type; };
template <> struct NsFwdArg<true, false> { typedef NsJvp type; };
template <> struct NsFwdArg<true, true> { typedef NsRefine type; };
template <> struct NsFwdArg<true, false, true> { typedef NsJvpQp type; };
template <> struct NsFwdArg<true, true, true> { typedef NsRefineQp type; };
template <> struct NsFwdArg<true, false, false, true> { typedef NsJvpTri type; };
template <> struct NsFwdArg<true, true, false, true> { typedef NsRefineTri type; };
template <> struct NsFwdArg<false, false, false, false, true> { typedef NsMany type; };
template <> struct NsFwdArg<true, false, false, false, true> { typedef NsJvpMany type; };
template <> struct NsFwdArg<true, false, true, false, true> { typedef NsJvpQpMany type; };
template <> struct NsFwdArg<false, false, true, false, true> { typedef NsVjpQpMany type; };
template <> struct NsFwdArg<false, false, false, true, true> { typedef NsVjpTriMany type; };
template <> struct NsFwdArg<true, false, false, true, true> { typedef NsJvpManyTri type; };
template <> struct NsFwdArg<true, false, false, false, false, true> { typedef NsJvpPsd type; };
template <> struct NsFwdArg<true, true, false, false, false, true> { typedef NsRefinePsd type; };
template <> struct NsFwdArg<false, false, false, false, true, true> { typedef NsVjpManyPsd type; };
template <> struct NsFwdArg<true, false, false, false, true, true> { typedef NsJvpManyPsd type; };
template <> struct NsFwdArg<true, false, false, true, false, true> { typedef NsJvpPsdTri type; };
template <> struct NsFwdArg<true, true, false, true, false, true> { typedef NsRefinePsdTri type; };
template <> struct NsFwdArg<false, false, false, true, true, true> { typedef NsVjpManyPsdTri type; };
template <> struct NsFwdArg<true, false, false, true, true, true> { typedef NsJvpManyPsdTri type; };

// (QP: 20 KB more LDS at the config-2 shape -- two workgroups per CU, and the registers that go with two; TRI: the triples' eigen-decompositions are calls with
// frames of their own, planned for two as well; PSD: the block's segments on top of A leave room for two at the shapes it serves)
template <int NTILE, int NTHR, bool FWD = false, bool REF = false, bool QP = false, bool TRI = false, bool MANY = false, bool PSD = false>
__global__ void __launch_bounds__(NTHR, (NTHR == 256 ? ((QP || TRI || PSD) ? 2 : 3) : 1))
k_backward_ns(DevT T, const double *__restrict__ Avals, const double *__restrict__ xg, const double *__restrict__ yg, const double *__restrict__ sg,
              const double *__restrict__ dxg, const double *__restrict__ dyg, double *__restrict__ dAo, double *__restrict__ dqo, long sdqk, long sdqb,
              int *__restrict__ adj_status, int *__restrict__ fix, typename NsFwdArg<FWD, REF, QP, TRI, MANY, PSD>::type W) {
    static_assert(FWD || !REF, "the refinement step is the forward derivative's elimination with its own prologue and epilogue");
    static_assert(FWD || !QP || MANY, "the single-cotangent adjoint with a quadratic objective lives in k_backward_rt");
    static_assert((FWD && !QP) || (!FWD && !REF && !QP && MANY) || !TRI,
                  "exponential / power triples: the forward modes with a linear objective (one tangent, many tangents, refinement), and the many-cotangent adjoint "
                  "with one (their single-cotangent adjoint lives in k_backward_rt)");
    static_assert(!MANY || (!FWD && !REF && !(TRI && QP) && !(PSD && QP)) || (FWD && !REF && !(TRI && QP) && !(PSD && QP)),
                  "many right-hand sides on one factorisation: the adjoint (K cotangents) or the forward derivative (K tangents), each with plain cones, P or not, or "
                  "with triples, PSD blocks or both and a linear objective; never the refinement, never triples or PSD blocks with P");
    static_assert(!PSD || (!QP && ((FWD && !MANY) || (MANY && !REF))),
                  "PSD blocks, triples beside them or not: the forward derivative and the refinement on one right-hand side, K tangents and K cotangents on one "
                  "factorisation; linear objective (their single-cotangent adjoint lives in k_backward_rt)");
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int NWB = NTHR / 64, LDP = bwd_ns_ldp(NTILE), NSL = bwd_ns_nsl(NTILE), NCOLP = 64 * NSL, PUBP = NCOLP + 2;
    constexpr int NLOC = (16 * NTILE - 4 + NWB - 1) / NWB;          // equality rows per wave (rows are dealt cyclically to the waves)
    static_assert(NWB >= NTILE, "one wave per 16-row strip of the reduced system");
    typedef double v4d __attribute__((ext_vector_type(4)));
    const int tid = threadIdx.x, inst = blockIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lg = lane >> 4, lc = lane & 15;
    const int n = T.n, m = T.m, lda = T.lda, nq = T.nq, z = T.z;
    const int nqs = nq > 0 ? nq : 1, npad = n + (n & 1), KWMAX = bwd_ns_kwmax(m);

    // ---- LDS carve
    double *p = sm;
    double *A = p; p += m * lda; p += (p - sm) & 1;
    double *vv = p; p += m;          // v = y - s ; later r_y
    double *dv = p; p += m;          // dy, then d = DPi dy ; later y (outputs)
    double *rx = p; p += npad;
    double *fvec = p; p += npad;     // f = dx + sum over boundary cones [...]; its free entries become Z^T f ; later x (outputs)
    double *dB = p; p += npad;       // right-hand side of the equalities -> d~ -> x_piv ; finally the multipliers mu
    double *cinfo = p; p += 5 * nqs; // per cone: lambda, |z|, e_y.d, e_s.d, theta
    double *tvec = p; p += KWMAX;    // per weighted row: t_k = a_k . x_p ; later q_k = a_k . r_x
    double *wgt = p; p += KWMAX;     // per weighted row: its weight in H (theta_c for the z-rows of cone c, -theta_c for a_z)
    double *red = p; p += NWB * 8;   // REF: the partial maxima of the residual norms, two per wave
    double *qaz = p; p += nqs;       // a_z . r_x per cone
    p += (p - sm) & 1;
    double *U = p; p += bwd_ns_union_doubles(n, m, nqs, NTILE);
    double *az = U;                  // a_z = A_z^T z-hat per boundary cone (pitch npad); dead after the Gram
    double *pub = U + nqs * npad;    // row elimination: two publication buffers {scaled pivot row (64 NSL), inverse pivot, pivot column}
    double *Rbuf = U;                // the sweep's two buffers of four rows
    double *qv2 = U;                 // (A r_x)_i for the rows of boundary cones, after the sweep
    double *mu = U + m + (m & 1);    // g = (H r_x - f)[piv] by equality index, after the sweep (the multipliers themselves end in dB)
    int *ip = (int *)p;
    int *rkind = ip; ip += m;
    int *eqrow = ip; ip += m;
    int *ckind = ip; ip += nqs;
    int *ceq = ip; ip += nqs;
    int *cbase = ip; ip += nqs;      // first entry of cone c in the weighted-row list
    int *erow = ip; ip += n;         // equality e -> offset of its row in sm
    int *pcol = ip; ip += n;         // equality e -> pivot column (-1: redundant row, dropped)
    int *cmap = ip; ip += n;         // column j -> free index f (>= 0) or -1 (pivot column)
    int *fcol = ip; ip += n;         // free index f -> column ; before the row elimination: equality e -> source (row index >= 0, or -1 - cone)
    int *esrc = fcol;
    int *wrow = ip; ip += KWMAX;     // weighted row -> offset of its row in sm
    int *wsrc = ip; ip += KWMAX;     // weighted row -> row index of A (>= 0) or -1 - cone (a_z)
    int *wcnt = ip; ip += NWB + 1;
    int *misc = ip; ip += 8;         // [0] n_eq, [1] nf, [2] flags, [3] KW
    double *Pm = nullptr, *ptv = nullptr; int *peq = nullptr;
    if constexpr (QP) {
        ip += (ip - (int *)sm) & 1;
        Pm = (double *)ip;           // P, dense and symmetric (pitch n); step 2 turns its rows into p~_j = Z^T p_j in the free columns
        ptv = Pm + n * n;            // per row of P: t_j = p_j . x_p
        peq = (int *)(ptv + npad);   // pivot column j -> its equality e
    }
    const int ntri = TRI ? T.nep + T.np : 0;
    double *Wt = nullptr, *lamt = nullptr;
    if constexpr (TRI) {
        ip += (ip - (int *)sm) & 1;
        Wt = (double *)ip;           // per triple: W (row-major 3 x 3, eigenvectors in the columns) of D Pi_K*(v)
        lamt = Wt + 9 * ntri;        // per rotated triple row: its eigenvalue after the snap
        if constexpr (PSD) ip = (int *)(lamt + 3 * ntri);          // (both kinds: the blocks' segments follow the triples', ns_layout's order)
    }
    // PSD: per block U and Lambda of smat(v_c), per rotated row its eigenvalue B of D Pi, the Jacobi scratch and one (X, W) pair per wave for the rotations (ns_layout's
    // PSD mode: nothing here aliases the union region).  The blocks' rows are psd0 .. T.eoff - 1; with TRI the triples' rows follow them, T.eoff .. m - 1.
    const int psd0 = PSD ? T.soff[0] : 0, msq = PSD ? T.maxs * T.maxs : 0;
    double *psdU = nullptr, *psdEv = nullptr, *lamp = nullptr, *psdScr = nullptr, *psdXW = nullptr;
    if constexpr (PSD) {
        ip += (ip - (int *)sm) & 1;
        psdU = (double *)ip;
        psdEv = psdU + T.ns * msq;
        lamp = psdEv + T.ns * T.maxs;
        psdScr = lamp + (T.eoff - psd0);
        psdXW = psdScr + 2 * msq + 2 * T.maxs + 8;
    }
    // QP: the instance's P row through the template's dense entry map (-1: structural zero; a one-triangle entry stands for both matrix entries)
    auto load_P = [&]() {
        if constexpr (QP) {
            const double *Pv = W.Q.P + (size_t)inst * W.Q.nnz_p;
            for (int i = tid; i < n * n; i += NTHR) { const int k = W.Q.pmap[i]; Pm[i] = k >= 0 ? Pv[k] : 0.0; }
        }
    };

#ifdef CE_TIMING
    __shared__ long long tstamp[16], tsub[16];
    if (threadIdx.x < 16) tsub[threadIdx.x] = 0;
#endif
    // ---- REF: the instance's record of this call.  An instance the forward solve failed on (16), one whose earlier step the safeguard rejected (2) or the
    //      elimination flagged (4) keeps its point bit for bit and takes no further step.  rho_cur: rho of the point as stored when it was written.
    int rst0 = 0; double rho_cur = 0.0, rho0 = 0.0;
    if constexpr (REF) {
        rst0 = W.first ? ((W.status && W.status[inst] < 0) ? 16 : 0) : W.rstatus[inst];
        if (!W.first) rho_cur = W.resid[2 * (size_t)inst + 1];
        if (W.first && tid == 0) {
            W.rstatus[inst] = rst0; W.steps[inst] = 0;
            if (rst0) { W.resid[2 * (size_t)inst] = __builtin_nan(""); W.resid[2 * (size_t)inst + 1] = __builtin_nan(""); }
        }
        if (rst0 & (2 | 4 | 16)) return;
    }
    // PSD: smat(v_c) = U Lambda U^T of every block by the workgroup's Jacobi sweeps (U -> psdU, vectors in the columns; Lambda -> psdEv).  ONE decomposition gives the
    // eigenvalues B of D Pi in the classification pass and, REF, y-hat of the block.  All threads; ends behind a barrier.
    auto psd_decompose = [&](const double *vs) {
        if constexpr (PSD) {
            for (int c = 0; c < T.ns; c++) {
                const int k = T.sord[c];
                psd_jacobi<NTHR>(vs + T.soff[c], k, psdScr, psdU + c * msq, psdScr + 2 * msq, red);
                for (int i = tid; i < k; i += NTHR) psdEv[c * T.maxs + i] = psdScr[i * k + i];
                __syncthreads();
            }
        }
    };
    // PSD with MANY: one block vector per right-hand side through the retained U, in place, every block in turn on the first (X, W) pair of psdXW (the rotation
    // workspace per right-hand side; psdScr idles behind the decomposition).  back == false:  r_c <- Q^T r_c = svec(U^T smat(r_c) U)  (gamma of a tangent, h of a
    // cotangent);  back == true:  r_c <- Q r_c = svec(U smat(r_c) U^T)  (r_y of a cotangent).  All threads; three phases per block behind barriers, the block loop
    // and the phases workgroup-uniform (T.ns, T.sord are the template's); the caller has a barrier in front, the last phase ends behind one.
    auto psd_rotate_vec = [&](double *vec, bool back) {
        if constexpr (PSD && MANY) {
            double *X = psdXW, *Wm = psdXW + msq;
            for (int c = 0; c < T.ns; c++) {
                const int k = T.sord[c], r0 = T.soff[c], d = k * (k + 1) / 2;
                const double *Um = psdU + c * msq;
                for (int idx = tid; idx < k * k; idx += NTHR) {
                    const int i = idx / k, j = idx - i * k, a = i >= j ? i : j, b = i >= j ? j : i;
                    const double v = vec[r0 + b * k - (b * (b - 1)) / 2 + (a - b)];
                    X[idx] = (a == b) ? v : v * M_SQRT1_2;
                }
                __syncthreads();
                for (int idx = tid; idx < k * k; idx += NTHR) {          // W = X U  (back: X U^T)
                    const int i = idx / k, j = idx - i * k;
                    double acc = 0; for (int a = 0; a < k; a++) acc = fma(X[i * k + a], back ? Um[j * k + a] : Um[a * k + j], acc);
                    Wm[idx] = acc;
                }
                __syncthreads();
                for (int pos = tid; pos < d; pos += NTHR) {              // U^T W  (back: U W), packed back as svec
                    int b = 0, rem = pos; while (rem >= k - b) { rem -= k - b; b++; }
                    const int a = b + rem;
                    double acc = 0; for (int i = 0; i < k; i++) acc = fma(back ? Um[a * k + i] : Um[i * k + a], Wm[i * k + b], acc);
                    vec[r0 + pos] = (a == b) ? acc : acc * M_SQRT2;
                }
                __syncthreads();
            }
        }
    };
    // REF: y-hat = the projection of v onto the dual cone (zero -> free, nonnegative, second-order) by ns_soc_kind, the decision of the classification pass below
    // (16 lanes per cone); s-hat = y-hat - v
    auto project_dual = [&](const double *vs, double *yh) {
        if constexpr (!REF) return;
        else {
        for (int i = tid; i < z + T.l; i += NTHR) { const double w = vs[i]; yh[i] = (i < z || w > 0) ? w : 0.0; }
        for (int c0 = 0; c0 < nq; c0 += NTHR / 16) {
            const int c = c0 + (tid >> 4), l16 = tid & 15;
            const bool cv = c < nq;
            const int r0 = cv ? T.qoff[c] : 0, r1 = cv ? T.qoff[c + 1] : 0, d = r1 - r0;
            const double t0 = cv ? vs[r0] : 0.0;
            double nz2 = 0.0;
            for (int i = r0 + 1 + l16; i < r1; i += 16) { const double w = vs[i]; nz2 = fma(w, w, nz2); }
            nz2 = group_reduce<16, false>(nz2);
            const double nz = sqrt(nz2);
            double lam;
            const int kind = ns_soc_kind(d, t0, nz, lam);
            if (kind == 0) lam = 1.0;          // Pi(v) = v inside the cone, 0 inside the polar, lam (nz, z) else
            for (int i = r0 + 1 + l16; i < r1; i += 16) yh[i] = lam * vs[i];
            if (cv && l16 == 0) yh[r0] = kind == 2 ? lam * nz : lam * t0;
        }
        if constexpr (TRI) {          // one thread per triple, from the cold start exp_dual_eig / pow_dual_eig evaluate at: the decision of the classification pass
            for (int c = tid; c < ntri; c += NTHR) {
                const int r0 = T.eoff + 3 * c;
                double w[3] = {vs[r0], vs[r0 + 1], vs[r0 + 2]};
                if (c < T.nep) { double rs = 0.0; exp_project_dual(w, &rs); } else { double rs = -1.0; pow_project_dual_of_entry(w, T.pw[c - T.nep], &rs); }
                yh[r0] = w[0]; yh[r0 + 1] = w[1]; yh[r0 + 2] = w[2];
            }
        }
        if constexpr (PSD) {          // y-hat_c = svec(U max(Lambda, 0) U^T) from the decomposition the classification pass reads its B from (psdU, psdEv): one decision
            psd_decompose(vs);
            for (int c = 0; c < T.ns; c++) {
                const int k = T.sord[c], r0 = T.soff[c];
                const double *Um = psdU + c * msq, *ev = psdEv + c * T.maxs;
                for (int pos = tid; pos < k * (k + 1) / 2; pos += NTHR) {
                    int b = 0, rem = pos; while (rem >= k - b) { rem -= k - b; b++; }
                    const int a = b + rem;
                    double acc = 0; for (int e = 0; e < k; e++) acc = fma(Um[a * k + e] * fmax(ev[e], 0.0), Um[b * k + e], acc);
                    yh[r0 + pos] = (a == b) ? acc : acc * M_SQRT2;
                }
            }
        }
        }
    };
    // REF: the KKT residual at (x, y-hat, s-hat) of the instance in A:  F_x = [P x +] A^T y-hat + c,  F_y = A x + s-hat - b  (b through bpos, c from q_eval); returns
    // rho = max(|F_x|, |F_y|) / (1 + max(|b|, |c|)), a non-finite entry counting as infinite.  keep: F_x -> fvec, -F_y -> dv (g_x, g_y of the elimination).
    // Four lanes per column / row, fixed summation order; ends behind a barrier.
    auto kkt_residual = [&](const double *xs, const double *yh, const double *vs, bool keep) -> double {
        if constexpr (!REF) return 0.0;
        else {
        const double *vals = Avals + (size_t)inst * T.nnz_aug;
        const double inf = __builtin_inf();
        double mx = 0.0, sc = 0.0;
        for (int j0 = 0; j0 < n; j0 += NTHR / 4) {
            const int j = j0 + (tid >> 2), part = tid & 3;
            double a0 = 0.0, a1 = 0.0;
            if (j < n) for (int i = part; i < m; i += 8) {
                const int i2 = min(i + 4, m - 1);
                const double r0v = A[i * lda + j], r1v = A[i2 * lda + j], y0 = yh[i], y1 = yh[i2];
                a0 = fma(r0v, y0, a0); a1 = fma(r1v, (i + 4 < m) ? y1 : 0.0, a1);
            }
            if constexpr (QP) { if (j < n) for (int i = part; i < n; i += 4) a0 = fma(Pm[j * n + i], xs[i], a0); }          // (P as loaded: untransformed at both evaluations)
            const double a = group_reduce<4, false>(a0 + a1);
            if (j < n && part == 0) {
                const double cj = W.q[j * W.sqk + inst * W.sqb], f = a + cj, fa = fabs(f);
                if (keep) fvec[j] = f;
                mx = fmax(mx, fa < inf ? fa : inf); sc = fmax(sc, fabs(cj));
            }
        }
        for (int i0 = 0; i0 < m; i0 += NTHR / 4) {
            const int i = i0 + (tid >> 2), part = tid & 3;
            double a0 = 0.0, a1 = 0.0;
            if (i < m) {
                const double *row = A + i * lda;
                for (int j = part; j < n; j += 8) {
                    const int j2 = min(j + 4, n - 1);
                    const double r0v = row[j], r1v = row[j2], x0 = xs[j], x1 = xs[j2];
                    a0 = fma(r0v, x0, a0); a1 = fma(r1v, (j + 4 < n) ? x1 : 0.0, a1);
                }
            }
            const double a = group_reduce<4, false>(a0 + a1);
            if (i < m && part == 0) {
                const int pb = W.bpos[i];
                const double bi = pb >= 0 ? vals[pb] : 0.0, f = a + (yh[i] - vs[i]) - bi, fa = fabs(f);
                if (keep) dv[i] = -f;
                mx = fmax(mx, fa < inf ? fa : inf); sc = fmax(sc, fabs(bi));
            }
        }
        mx = wave_reduce_dpp<true>(mx); sc = wave_reduce_dpp<true>(sc);
        if (lane == 0) { red[2 * wave] = mx; red[2 * wave + 1] = sc; }
        __syncthreads();
        double mxa = 0.0, sca = 0.0;
#pragma unroll
        for (int w = 0; w < NWB; w++) { mxa = fmax(mxa, red[2 * w]); sca = fmax(sca, red[2 * w + 1]); }
        __syncthreads();
        return mxa / (1.0 + sca);
        }
    };
    // ---- FWD prologue: g = dQ pi without its tau entry,  g_x = dc + dA^T y [+ dP x] -> fvec,  g_y = db - dA x -> dv,  with the tangents in the boundary convention
    //      (k_sa_lsqr<FWD>'s prologue: dA = -tA_eval, db = +tA_eval[bpos], dc = tq_eval[:n]).  The instance's tangent row is read through the template's CSC
    //      (the value order itself) and CSR structure, 8 lanes per column / row, four entries in flight per lane; fixed summation order.
    //      tA, tP: the instance's tangent rows; tq: its tangent of q_eval, entry j at tq[j * tqs]; NULL: zero.  MANY calls it once per tangent.
    auto fwd_prologue = [&](const double *tA, const double *tq, long tqs, const double *tP) {
        if constexpr (!FWD || REF) return;
        else {
        for (int j0 = 0; j0 < n; j0 += NTHR / 8) {
            const int j = j0 + (tid >> 3), c8 = tid & 7;
            double a0 = 0.0, a1 = 0.0;
            if (tA && j < n) {
                const int k1 = W.csc_ptr[j + 1];
                for (int k = W.csc_ptr[j] + c8; k < k1; k += 32) {
                    double tv[4]; int ri[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) { const int kk = min(k + 8 * u, k1 - 1); tv[u] = tA[kk]; ri[u] = T.rowidx[kk]; }
#pragma unroll
                    for (int u = 0; u < 4; u++) { const double t = (k + 8 * u < k1) ? tv[u] : 0.0; if (u & 1) a1 = fma(t, tvec[ri[u]], a1); else a0 = fma(t, tvec[ri[u]], a0); }
                }
            }
            double as = a0 + a1;
            if constexpr (QP) {          // - (tP x)_j: row j of the tangent of P through the dense entry map
                if (tP && j < n) {
                    double pa = 0.0;
                    for (int i = c8; i < n; i += 8) { const int k = W.Q.pmap[j * n + i]; pa = fma(k >= 0 ? tP[k >= 0 ? k : 0] : 0.0, rx[i], pa); }
                    as -= pa;
                }
            }
            const double a = group_reduce<8, false>(as);
            if (j < n && c8 == 0) fvec[j] = (tq ? tq[j * tqs] : 0.0) - a;
        }
        for (int i0 = 0; i0 < m; i0 += NTHR / 8) {
            const int i = i0 + (tid >> 3), c8 = tid & 7;
            double a0 = 0.0, a1 = 0.0;
            if (tA && i < m) {
                const int k1 = W.csr_ptr[i + 1];
                for (int k = W.csr_ptr[i] + c8; k < k1; k += 32) {
                    double tv[4]; int ci[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) { const int kk = min(k + 8 * u, k1 - 1); tv[u] = tA[W.csr_src[kk]]; ci[u] = W.csr_col[kk]; }
#pragma unroll
                    for (int u = 0; u < 4; u++) { const double t = (k + 8 * u < k1) ? tv[u] : 0.0; if (u & 1) a1 = fma(t, rx[ci[u]], a1); else a0 = fma(t, rx[ci[u]], a0); }
                }
            }
            const double a = group_reduce<8, false>(a0 + a1);
            if (i < m && c8 == 0) { const int pb = tA ? W.bpos[i] : -1; dv[i] = (pb >= 0 ? tA[pb] : 0.0) + a; }
        }
        }
    };
    NS_STAMP(0);
    // ---- load: the instance's values scattered into dense solver form A = -A_cvx (b is not needed: r_tau is pinned)
    {
        constexpr int LU = NTHR == 256 ? 20 : 12;
        const double *vals = Avals + (size_t)inst * T.nnz_aug;
        const int nnz = T.nnzA;
        double v0[LU]; int r0[LU], c0[LU];
#pragma unroll
        for (int u = 0; u < LU; u++) { const int k = tid + u * NTHR, kc = k < nnz ? k : 0; v0[u] = vals[kc]; r0[u] = T.rowidx[kc]; c0[u] = k < nnz ? T.colidx[kc] : -1; }
        for (int i = tid; i < m * lda; i += NTHR) A[i] = 0.0;
        if constexpr (REF) {          // (in / out arrays: read through the pointers they are written through)
            for (int i = tid; i < m; i += NTHR) vv[i] = W.y[(size_t)inst * m + i] - W.s[(size_t)inst * m + i];
            for (int j = tid; j < n; j += NTHR) rx[j] = W.x[(size_t)inst * n + j];
        } else if constexpr (FWD && MANY) {          // (steps 1-4 on a zero right-hand side: g_y = 0 here, f = 0 below; every tangent comes behind the sweep)
            for (int i = tid; i < m; i += NTHR) { vv[i] = yg[(size_t)inst * m + i] - sg[(size_t)inst * m + i]; dv[i] = 0.0; }
        } else if constexpr (FWD) {          // (y and x wait in tvec and rx for the tangent products of the prologue below)
            for (int i = tid; i < m; i += NTHR) { const double yi = yg[(size_t)inst * m + i]; vv[i] = yi - sg[(size_t)inst * m + i]; tvec[i] = yi; }
            for (int j = tid; j < n; j += NTHR) rx[j] = xg[(size_t)inst * n + j];
        } else
        for (int i = tid; i < m; i += NTHR) { vv[i] = yg[(size_t)inst * m + i] - sg[(size_t)inst * m + i]; if constexpr (MANY) dv[i] = 0.0; else dv[i] = dyg[(size_t)inst * m + i]; }
        if (tid < 8) misc[tid] = 0;
        load_P();
        __syncthreads();
#pragma unroll
        for (int u = 0; u < LU; u++) if (c0[u] >= 0) A[r0[u] * lda + c0[u]] = -v0[u];
        for (int kb = LU * NTHR; kb < nnz; kb += LU * NTHR) {
#pragma unroll
            for (int u = 0; u < LU; u++) { const int k = kb + tid + u * NTHR, kc = k < nnz ? k : 0; v0[u] = vals[kc]; r0[u] = T.rowidx[kc]; c0[u] = k < nnz ? T.colidx[kc] : -1; }
#pragma unroll
            for (int u = 0; u < LU; u++) if (c0[u] >= 0) A[r0[u] * lda + c0[u]] = -v0[u];
        }
        __syncthreads();
    }
    if constexpr (REF) {
        // ---- REF prologue: the residual map itself in the place of dQ pi:  g_x = F_x -> fvec,  g_y = -F_y -> dv,  evaluated at the complementary pair
        //      y-hat = Pi(v) (-> tvec), s-hat = y-hat - v, never at the caller's y, s;  rho before the step
        project_dual(vv, tvec);
        __syncthreads();
        rho0 = kkt_residual(rx, tvec, vv, true);
        if (W.first) rho_cur = rho0;
    } else if constexpr (FWD && !MANY) {
        fwd_prologue(W.tA ? W.tA + (size_t)inst * T.nnz_aug : nullptr, W.tq ? W.tq + inst * W.stqb : nullptr, W.stqk, [&]() -> const double * {
            if constexpr (QP) return W.Q.tP ? W.Q.tP + (size_t)inst * W.Q.nnz_p : nullptr; else return nullptr; }());
        __syncthreads();
    }
    NS_STAMP(1);
    // ---- classify + d = DPi(v) dy in ONE pass: 16 lanes per cone (a row per lane, sums by DPP butterflies inside the 16-lane row), nonnegative rows beside them.
    //      (One thread per cone walked its rows in dependent loops: 8 of 256 threads busy, ~25 k cycles for the two phases.)  dv holds dy: transformed in place.
    for (int i = tid; i < z + T.l; i += NTHR) { const bool eq = (i < z || vv[i] > 0); rkind[i] = eq ? RK_EQ : RK_FREE; if constexpr (!FWD) if (!eq) dv[i] = 0.0; }
    for (int c0 = 0; c0 < nq; c0 += NTHR / 16) {
        const int c = c0 + (tid >> 4), l16 = tid & 15;
        const bool cv = c < nq;
        const int r0 = cv ? T.qoff[c] : 0, r1 = cv ? T.qoff[c + 1] : 0, d = r1 - r0;
        const double t0 = cv ? vv[r0] : 0.0, h0 = cv ? dv[r0] : 0.0;
        double nz2 = 0.0, zh = 0.0;
        for (int i = r0 + 1 + l16; i < r1; i += 16) { const double w = vv[i]; nz2 = fma(w, w, nz2); zh = fma(w, dv[i], zh); }
        nz2 = group_reduce<16, false>(nz2); zh = group_reduce<16, false>(zh);
        const double nz = sqrt(nz2);
        double lam;
        const int kind = ns_soc_kind(d, t0, nz, lam);
        double zd = 0.0;
        const double i2n = kind == 2 ? 1.0 / (2 * nz) : 0.0, cz = kind == 2 ? t0 * zh / (nz * nz) : 0.0;
        const int rk = kind == 0 ? RK_EQ : (kind == 1 ? RK_FREE : RK_SOCB);
        if constexpr (FWD) {
            // the rows keep g_y (the epilogue wants it unrotated); per boundary cone gamma_y = e_y . g, gamma_s = e_s . g (cinfo[2], cinfo[3]) and the weights
            // u_i = theta (g_i - z-hat_i (z-hat . g_z)) of the cone's z-rows in  f + g_x = sum theta a~^T gamma = A^T u  (tvec; 0 on the t-row)
            for (int i = r0 + 1 + l16; i < r1; i += 16) rkind[i] = rk;
            if (kind == 2) {
                const double zeta = zh / nz, th = lam / (1 - lam), inz = 1.0 / nz;
                for (int i = r0 + 1 + l16; i < r1; i += 16) tvec[i] = th * (dv[i] - vv[i] * inz * zeta);
                if (l16 == 0) { tvec[r0] = 0.0; cinfo[5 * c + 2] = (h0 + zeta) * M_SQRT1_2; cinfo[5 * c + 3] = (h0 - zeta) * M_SQRT1_2; }
            }
            if (cv && l16 == 0) { rkind[r0] = rk; ckind[c] = kind; cinfo[5 * c] = lam; cinfo[5 * c + 1] = nz; cinfo[5 * c + 4] = lam / (1 - lam); }
            continue;
        }
        for (int i = r0 + 1 + l16; i < r1; i += 16) {
            rkind[i] = rk;
            if (kind == 1) dv[i] = 0.0;
            else if (kind == 2) { const double w = vv[i]; const double di = (w * h0 + (t0 + nz) * dv[i] - w * cz) * i2n; dv[i] = di; zd = fma(w, di, zd); }
        }
        zd = group_reduce<16, false>(zd);
        if (kind == 2) {
            // u_i: the weight of row i of this cone in  f - dx = sum_c [ a_s (e_s.d) + (A_c^T d - a_y (e_y.d) - a_s (e_s.d)) / (1 - lam) ] = A^T u  (a_y, a_s are
            // combinations of the cone's rows: a_y = (a_0 + a_z) / sqrt 2, a_s = (a_0 - a_z) / sqrt 2, a_z = A_z^T z-hat), so that f is ONE pass over the rows
            // together with a_z, not a pass of its own behind a_z and a barrier
            const double d0 = (nz * h0 + zh) * i2n, zdn = zd / nz, eyd = (d0 + zdn) * M_SQRT1_2, esd = (d0 - zdn) * M_SQRT1_2;
            const double il = 1.0 / (1 - lam), k0c = (esd * (1 - il) - eyd * il) * M_SQRT1_2, kzc = (-esd * (1 - il) - eyd * il) * M_SQRT1_2, inz = 1.0 / nz;
            for (int i = r0 + 1 + l16; i < r1; i += 16) tvec[i] = fma(il, dv[i], vv[i] * inz * kzc);
            if (l16 == 0) tvec[r0] = fma(il, d0, k0c);
        }
        if (cv && l16 == 0) {
            rkind[r0] = rk; ckind[c] = kind; cinfo[5 * c] = lam; cinfo[5 * c + 1] = nz; cinfo[5 * c + 4] = lam / (1 - lam);
            if (kind == 1) dv[r0] = 0.0;
            else if (kind == 2) {
                const double d0 = (nz * h0 + zh) * i2n;
                dv[r0] = d0;
                const double zdn = zd / nz;
                cinfo[5 * c + 2] = (d0 + zdn) * M_SQRT1_2;   // e_y . d
                cinfo[5 * c + 3] = (d0 - zdn) * M_SQRT1_2;   // e_s . d
            }
        }
    }
    if constexpr (TRI) {
        // triples: S = D Pi_K*(v_c) = W diag(lambda) W^T, one thread per triple; lambda snapped as k_backward_rt snaps it (the same constants: both kernels
        // decide alike).  The rows keep gamma = W^T g_y (dv); a weighted row's share of f, theta gamma, waits in tvec like the u_i of a boundary cone.
        for (int c = tid; c < ntri; c += NTHR) {
            const int r0 = T.eoff + 3 * c;
            double Wl[9], th[3];
            if (c < T.nep) exp_dual_eig(vv + r0, Wl, th); else pow_dual_eig(vv + r0, T.pw[c - T.nep], Wl, th);
            const double h0 = dv[r0], h1 = dv[r0 + 1], h2 = dv[r0 + 2];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const double t = Wl[a] * h0 + Wl[3 + a] * h1 + Wl[6 + a] * h2;     // (W^T g_y)_a
                double Bv = th[a];
                if (Bv < 1e-9) Bv = 0.0; else if (Bv > 1.0 - 1e-9) Bv = 1.0;
                const bool mix = Bv != 1.0 && Bv != 0.0;
                // a weighted row that is all but an equality (1 - lambda < NS_TRI_STIFF, theta > 1e5): the reduced Hessian carries theta, the sweep has no pivot search
                // and eta divides by 1 - lambda again -- measured on the MI355X the error of such an instance grows like 0.03 eps theta^2 (1e-1 at 1 - lambda = 3e-9,
                // 4e-7 at 8e-7, 1e-10 at 1e-4).  The forward derivative flags it like a rank-deficient instance and the re-solve behind ce_jvp serves it; a Newton
                // step needs no such accuracy (an inexact step still contracts, and the safeguard judges it by rho): ce_refine takes it.
                if constexpr (!REF) { if (mix && 1 - Bv < NS_TRI_STIFF) atomicOr(&misc[2], 4); }
                lamt[3 * c + a] = Bv; dv[r0 + a] = t; tvec[r0 + a] = mix ? Bv / (1 - Bv) * t : 0.0;
                rkind[r0 + a] = (Bv == 1.0) ? RK_EQ : (Bv == 0.0 ? RK_FREE : RK_MIX);
            }
#pragma unroll
            for (int k = 0; k < 9; k++) Wt[9 * c + k] = Wl[k];
        }
    }
    if constexpr (PSD) {
        // PSD blocks (as k_backward_rt<PSD>): in the orthonormal basis E_ab = svec(sym(u_a u_b^T)) D Pi(v_c) is diagonal with eigenvalue B_ab -- 1 when both
        // eigenvalues of smat(v_c) are positive, 0 when both are non-positive, l+ / (l+ - l-) otherwise (k_backward_rt's comparisons, no snap: both kernels decide
        // alike).  The block's rows of A are ROTATED into that basis in place, a~ = svec(U^T smat(a) U) per column, and gamma = Q^T g_y with them as column n (dv);
        // afterwards a rotated row is an ordinary equality (B = 1), a dropped row (B = 0) or ONE weighted row of the list (theta = B / (1 - B), theta gamma a~ in f:
        // tvec), exactly a triple's rows.  One column per wave at a time, on the wave's (X, W) pair.  REF: the decomposition is the prologue's (project_dual).
        if constexpr (!REF) psd_decompose(vv);
        for (int c = 0; c < T.ns; c++) {
            const int k = T.sord[c], r0 = T.soff[c], d = k * (k + 1) / 2;
            const double *Um = psdU + c * msq, *ev = psdEv + c * T.maxs;
            double *X = psdXW + wave * 2 * msq, *Wm = X + msq;
            for (int g0 = 0; g0 <= n; g0 += NWB) {
                const int col = g0 + wave;
                if (col <= n) {
                    for (int idx = lane; idx < k * k; idx += 64) {
                        const int i = idx / k, j = idx - i * k, a = i >= j ? i : j, b = i >= j ? j : i;
                        const int pos = b * k - (b * (b - 1)) / 2 + (a - b);
                        const double v = (col < n) ? A[(r0 + pos) * lda + col] : dv[r0 + pos];
                        X[idx] = (a == b) ? v : v * M_SQRT1_2;
                    }
                }
                __syncthreads();
                if (col <= n) {
                    for (int idx = lane; idx < k * k; idx += 64) {       // W = X U
                        const int i = idx / k, j = idx - i * k;
                        double acc = 0; for (int a = 0; a < k; a++) acc = fma(X[i * k + a], Um[a * k + j], acc);
                        Wm[idx] = acc;
                    }
                }
                __syncthreads();
                if (col <= n) {
                    for (int pos = lane; pos < d; pos += 64) {           // U^T W, packed back as svec
                        int b = 0, rem = pos; while (rem >= k - b) { rem -= k - b; b++; }
                        const int a = b + rem;
                        double acc = 0; for (int i = 0; i < k; i++) acc = fma(Um[i * k + a], Wm[i * k + b], acc);
                        const double t = (a == b) ? acc : acc * M_SQRT2;
                        if (col < n) A[(r0 + pos) * lda + col] = t;
                        else {
                            const double la = ev[a], lb = ev[b];
                            const double Bv = (la > 0 && lb > 0) ? 1.0 : ((la <= 0 && lb <= 0) ? 0.0 : fmax(la, lb) / (fmax(la, lb) - fmin(la, lb)));
                            const bool mix = Bv != 1.0 && Bv != 0.0;
                            // a weighted row that is all but an equality: the triples' rule and constant (NS_TRI_STIFF), carried over -- the law behind it is a property
                            // of the sweep, not of the cone, but it was not measured on PSD rows.  The forward derivative flags the instance, the refinement takes it.
                            if constexpr (!REF) { if (mix && 1 - Bv < NS_TRI_STIFF) atomicOr(&misc[2], 4); }
                            lamp[r0 - psd0 + pos] = Bv; dv[r0 + pos] = t; tvec[r0 + pos] = mix ? Bv / (1 - Bv) * t : 0.0;
                            rkind[r0 + pos] = (Bv == 1.0) ? RK_EQ : (Bv == 0.0 ? RK_FREE : RK_MIX);
                        }
                    }
                }
                __syncthreads();
            }
        }
    }
    __syncthreads();
    if constexpr (TRI) {          // A_c <- W^T A_c in place (read again behind the barriers of the numbering below)
        for (int idx = tid; idx < ntri * n; idx += NTHR) {
            const int c = idx / n, j = idx - c * n, r0 = T.eoff + 3 * c;
            const double *Wl = Wt + 9 * c;
            const double a0 = A[r0 * lda + j], a1 = A[(r0 + 1) * lda + j], a2 = A[(r0 + 2) * lda + j];
#pragma unroll
            for (int a = 0; a < 3; a++) A[(r0 + a) * lda + j] = Wl[a] * a0 + Wl[3 + a] * a1 + Wl[6 + a] * a2;
        }
    }
    NS_STAMP(2);
    // ---- equality numbering: ballot prefix sums (rows in order, then one e_y row per boundary cone); weighted-row list offsets
    {
        int base = 0;
        for (int i0 = 0; i0 < m; i0 += NTHR) {
            const int i = i0 + tid;
            const bool f = (i < m) && (rkind[i] == RK_EQ);
            const unsigned long long bal = __ballot(f);
            if (lane == 0) wcnt[wave] = __popcll(bal);
            __syncthreads();
            int off = base;
            for (int w = 0; w < wave; w++) off += wcnt[w];
            int tot = 0;
            for (int w = 0; w < NWB; w++) tot += wcnt[w];
            if (i < m) {
                const int e = f ? off + __popcll(bal & ((1ull << lane) - 1ull)) : -1;
                eqrow[i] = e;
                if (f && e < n) { esrc[e] = i; erow[e] = (int)(A - sm) + i * lda; }
            }
            base += tot;
            __syncthreads();
        }
        // one lane per cone: the boundary cones before it give its equality index and the start of its weighted rows
        for (int c = tid; c < nq; c += NTHR) {
            int ne = base, kw = 0;
            for (int c2 = 0; c2 < c; c2++) { if (ckind[c2] == 2) { ne++; kw += T.qoff[c2 + 1] - T.qoff[c2]; } }
            if (ckind[c] == 2) {
                if (ne < n) { esrc[ne] = -1 - c; erow[ne] = (int)(A - sm) + T.qoff[c] * lda; }      // (the cone's t-row will hold a_y)
                ceq[c] = ne; cbase[c] = kw;
                ne++; kw += T.qoff[c + 1] - T.qoff[c];
            } else { ceq[c] = -1; cbase[c] = -1; }
            if (c == nq - 1) { misc[0] = ne; misc[3] = kw; }
        }
        if (nq == 0 && tid == 0) { misc[0] = base; misc[3] = 0; }
        __syncthreads();
        if constexpr (TRI) {
            // the weighted rows of the triples follow the boundary cones' in the list, one lane per triple: entry, source row and weight theta at once (the rotated
            // row is in place already); eqrow of such a row keeps its list entry for the epilogue
            const int kw0 = misc[3];
            __syncthreads();
            for (int c = tid; c < ntri; c += NTHR) {
                int kw = kw0;
                for (int r = T.eoff; r < T.eoff + 3 * c; r++) kw += rkind[r] == RK_MIX ? 1 : 0;
                for (int a = 0; a < 3; a++) {
                    const int i = T.eoff + 3 * c + a;
                    if (rkind[i] != RK_MIX) continue;
                    const double lam = lamt[3 * c + a];
                    wrow[kw] = (int)(A - sm) + i * lda; wsrc[kw] = i; wgt[kw] = lam / (1 - lam); eqrow[i] = kw;
                    kw++;
                }
                if (c == ntri - 1) misc[3] = kw;
            }
            __syncthreads();
        }
        if constexpr (PSD) {
            // the weighted rows of the PSD blocks follow the boundary cones' in the list in row order, one lane per rotated row: entry, source row and weight theta (the
            // rotated row is in place already); eqrow of such a row keeps its list entry for the epilogue
            const int kw0 = misc[3];
            __syncthreads();
            for (int i = psd0 + tid; i < T.eoff; i += NTHR) {
                int kw = kw0;
                for (int r = psd0; r < i; r++) kw += rkind[r] == RK_MIX ? 1 : 0;
                if (rkind[i] == RK_MIX) {
                    const double lam = lamp[i - psd0];
                    wrow[kw] = (int)(A - sm) + i * lda; wsrc[kw] = i; wgt[kw] = lam / (1 - lam); eqrow[i] = kw;
                    kw++;
                }
                if (i == T.eoff - 1) misc[3] = kw;
            }
            __syncthreads();
        }
    }
    const int neq = misc[0], KW = misc[3], KW4 = (KW + 4) & ~3;          // (at least one pad entry: entry KW stands for f in the null-space transform)
    if (neq > n) {   // more active rows than variables: rank deficient by counting (flagged, zero gradient / zero tangents; the LSQR launch behind this kernel serves it)
        if constexpr (REF) {
            if (tid == 0) { W.rstatus[inst] = rst0 | 4; if (W.first) W.resid[2 * (size_t)inst] = rho0; W.resid[2 * (size_t)inst + 1] = rho_cur; }
        } else if constexpr (FWD && MANY) {          // (for every tangent; the instance is listed once)
            for (int kc = 0; kc < W.K; kc++) {
                for (int j = tid; j < n; j += NTHR) W.dx[kc * W.sxk + (size_t)inst * n + j] = 0.0;
                for (int i = tid; i < m; i += NTHR) { W.dy[kc * W.syk + (size_t)inst * m + i] = 0.0; if (W.ds) W.ds[kc * W.syk + (size_t)inst * m + i] = 0.0; }
                if (tid == 0) { if (W.iters) W.iters[kc * W.sak + inst] = 0; if (adj_status) adj_status[kc * W.sak + inst] = QP ? 4 : 2; }
            }
        } else if constexpr (FWD) {
            for (int j = tid; j < n; j += NTHR) W.dx[(size_t)inst * n + j] = 0.0;
            for (int i = tid; i < m; i += NTHR) { W.dy[(size_t)inst * m + i] = 0.0; if (W.ds) W.ds[(size_t)inst * m + i] = 0.0; }
            if (tid == 0 && W.iters) W.iters[inst] = 0;
        } else if constexpr (MANY) {          // (for every cotangent; the instance is listed once)
            for (int kc = 0; kc < W.K; kc++) {
                const bool records = W.rec != nullptr;          // (record mode, every many-cotangent kind: a zero record instead of the zero row -- and no dP, which is null then)
                if (records) { for (int k = tid; k < m + 1 + n; k += NTHR) W.rec[kc * W.srk + (size_t)inst * W.rpitch + k] = 0.0; }
                else
                for (int k = tid; k < T.nnz_aug; k += NTHR) dAo[kc * W.sAk + (size_t)inst * T.nnz_aug + k] = 0.0;
                for (int j = tid; j <= n; j += NTHR) dqo[kc * W.sqk + j * sdqk + inst * sdqb] = 0.0;
                if constexpr (QP) { if (!records) for (int k = tid; k < W.Q.nnz_p; k += NTHR) W.dP[kc * W.sPk + (size_t)inst * W.Q.nnz_p + k] = 0.0; }
                if (tid == 0 && adj_status) adj_status[kc * W.sak + inst] = QP ? 4 : 2;
            }
        } else {
            for (int k = tid; k < T.nnz_aug; k += NTHR) dAo[(size_t)inst * T.nnz_aug + k] = 0.0;
            for (int j = tid; j <= n; j += NTHR) dqo[j * sdqk + inst * sdqb] = 0.0;
        }
        if (tid == 0) { if constexpr (!MANY) { if (adj_status) adj_status[inst] = QP ? 4 : 2; } if (fix) fix[1 + atomicAdd(fix, 1)] = inst; }          // (QP: no re-solve behind the launch, the zeros stand, flagged)
        return;
    }
    // ---- f = dx + A^T u  and  a_z = A_z^T z-hat  in ONE pass over the rows of the boundary cones (4 lanes per column, each takes every 4th cone; fixed summation order)
    for (int j0 = 0; j0 < n; j0 += NTHR / 4) {
        const int j = j0 + (tid >> 2), part = tid & 3;
        double acc = 0;
        if (j < n) {
            for (int c = part; c < nq; c += 4) {
                if (ckind[c] != 2) continue;
                const int r0 = T.qoff[c], r1 = T.qoff[c + 1];
                double g = 0, g1 = 0, a = 0, a1 = 0;
                for (int i = r0; i < r1; i += 4) {
                    double av[4], uv[4], wv[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) { const int iu = min(i + u, r1 - 1); av[u] = A[iu * lda + j]; uv[u] = tvec[iu]; wv[u] = vv[iu]; }
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const bool in = i + u < r1;
                        const double uu = in ? uv[u] : 0.0, ww = (in && i + u > r0) ? wv[u] : 0.0;
                        if (u & 1) { g1 = fma(av[u], uu, g1); a1 = fma(av[u], ww, a1); } else { g = fma(av[u], uu, g); a = fma(av[u], ww, a); }
                    }
                }
                az[c * npad + j] = (a + a1) / cinfo[5 * c + 1];
                acc += g + g1;
            }
            if constexpr (TRI) {          // + theta gamma a~ of the triples' weighted rows
                for (int i = T.eoff + part; i < m; i += 4) if (rkind[i] == RK_MIX) acc = fma(A[i * lda + j], tvec[i], acc);
            }
            if constexpr (PSD) {          // + theta gamma a~ of the PSD blocks' weighted rows
                for (int i = psd0 + part; i < T.eoff; i += 4) if (rkind[i] == RK_MIX) acc = fma(A[i * lda + j], tvec[i], acc);
            }
        }
        acc = group_reduce<4, false>(acc);
        if constexpr (FWD && !MANY) { if (j < n && part == 0) fvec[j] = acc - fvec[j]; }          // f = -g_x + sum theta a~^T gamma
        else if constexpr (MANY) { if (j < n && part == 0) fvec[j] = acc; }          // (steps 1-4 run on a zero right-hand side: every cotangent comes behind the sweep)
        else
        if (j < n && part == 0) fvec[j] = acc + dxg[(size_t)inst * n + j];
    }
    __syncthreads();
    // ---- the e_y row of every boundary cone overwrites the cone's t-row (H does not contain the t-row: theta A_c^T (I - e_y e_y^T - e_s e_s^T) A_c =
    //      theta (A_z^T A_z - a_z a_z^T)); right-hand sides of the equalities; the weighted-row list {z-rows (theta), a_z (-theta)} per boundary cone
    for (int idx = tid; idx < nq * n; idx += NTHR) {
        const int c = idx / n, j = idx - c * n;
        if (ckind[c] != 2) continue;
        const int r0 = T.qoff[c];
        A[r0 * lda + j] = (A[r0 * lda + j] + az[c * npad + j]) * M_SQRT1_2;
    }
    for (int e = tid; e < neq; e += NTHR) { const int src = esrc[e]; dB[e] = src >= 0 ? dv[src] : cinfo[5 * (-1 - src) + 2]; }
    for (int i = tid; i < m; i += NTHR) {
        const int c = (i >= z + T.l && nq > 0) ? T.rowcone[i] : -1;
        if (c >= 0 && ckind[c] == 2) {
            const int r0 = T.qoff[c], r1 = T.qoff[c + 1];
            const double th = cinfo[5 * c + 4];
            if (i > r0) { const int q = cbase[c] + (i - r0 - 1); wrow[q] = (int)(A - sm) + i * lda; wsrc[q] = i; wgt[q] = th; }
            else { const int q = cbase[c] + (r1 - r0 - 1); wrow[q] = (int)(az - sm) + c * npad; wsrc[q] = -1 - c; wgt[q] = -th; }
        }
    }
    for (int q = KW + tid; q < KW4; q += NTHR) { wrow[q] = (int)(fvec - sm); wsrc[q] = -1 - nq; wgt[q] = 0.0; tvec[q] = 0.0; }      // entry KW = f (transformed like a row, weight 0), then pads to a multiple of four
    for (int j = tid; j < n; j += NTHR) { rx[j] = 0.0; cmap[j] = 0; }
    __syncthreads();
    NS_STAMP(3);
    // ---- 1. reduced row-echelon form of [B | d_B] with column pivoting.  The equality rows are dealt cyclically to the waves and live in REGISTERS (lane = column,
    //      column n = the right-hand side); per pivot the owner of the row finds the pivot column (DPP butterfly on |value| keys), publishes the scaled row, and
    //      after ONE barrier every wave updates its rows (multipliers by v_readlane from the pivot column's lane).  The pivot column keeps the multipliers and is
    //      carried through the later steps like any other column: it ends as column e of B_1^-1 (in-place Gauss-Jordan inversion), which mu needs.
    constexpr int NR1 = 24;          // equality rows one wave holds in registers (single-wave elimination: no barrier, no LDS traffic per pivot)
    if (NSL == 1 && neq <= NR1) {
        // Up to 24 equalities (metric configuration: ~17, i.e. ~9 active bounds + one e_y row per boundary cone): wave 0 keeps ALL rows in registers and runs the
        // whole elimination alone -- per pivot a DPP butterfly, one reciprocal and two v_readlane + one FMA per row; the other waves wait at the barrier behind it.
        // Rows are updated in groups of eight behind ONE uniform test (rows past neq hold zeros and are harmless to update): a scalar branch per row made a pivot
        // cost 2.8 k cycles, mostly branch latency.
        if (wave == 0) {          // (spreading this phase over the SIMDs by hardware wave slot was measured: no change -- it is bound by its own dependent chain, ~1.1 k cycles per pivot)
            double c1[NR1]; float rt1[NR1];
            static_for<NR1>([&](auto kc) {
                constexpr int kk = decltype(kc)::value;
                const double *ptr = sm + (kk < neq ? erow[kk < neq ? kk : 0] : 0);
                const double v = (kk < neq && lane < n) ? ptr[lane < n ? lane : 0] : 0.0;
                c1[kk] = (kk < neq && lane == n) ? dB[kk < neq ? kk : 0] : v;
                rt1[kk] = (float)fabs(v);
            });
            static_for<NR1 / 8>([&](auto gc) {          // rank tolerance of a row: CE_RANK_TOL x its largest entry as loaded (kept in single precision: a threshold)
                constexpr int g = decltype(gc)::value;
                if (8 * g < neq) {
                    static_for<8>([&](auto kc) {
                        constexpr int kk = 8 * g + decltype(kc)::value;
                        const double rmax = wave_reduce_dpp<true>((double)rt1[kk]);
                        rt1[kk] = (float)(CE_RANK_TOL * (rmax > 0 ? rmax : 1.0));
                    });
                }
            });
            bool cfr = true;
#ifdef CE_TIMING
            long long pacc[4] = {0, 0, 0, 0}, pt0 = __builtin_readcyclecounter();
#define NS_PACC(k) do { const long long t1_ = __builtin_readcyclecounter(); pacc[k] += t1_ - pt0; pt0 = t1_; } while (0)
#else
#define NS_PACC(k) do { } while (0)
#endif
            static_for<NR1>([&](auto ec) {
                constexpr int e = decltype(ec)::value;
                if (e < neq) {          // (uniform)
                    NS_PACC(3);
                    const double rv = c1[e];
                    const double key = __hiloint2double(__double2hiint(rv) & 0x7fffffff, (__double2loint(rv) & ~0xFF) | (255 - lane));
                    const double best = wave_reduce_dpp<true>((lane < n && cfr) ? key : 0.0);
                    const int jb = 255 - (__double2loint(best) & 0xFF);
                    const bool ok = best >= (double)rt1[e] && jb < n;
                    NS_PACC(0);
                    if (ok) {
                        const double pv = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(rv), jb), __builtin_amdgcn_readlane(__double2loint(rv), jb));
                        double inv = __builtin_amdgcn_rcp(pv);
                        inv = fma(fma(-pv, inv, 1.0), inv, inv);
                        inv = fma(fma(-pv, inv, 1.0), inv, inv);
                        const bool isj = lane == jb;
                        // The scaled pivot row carries 1 + 1/p (instead of 1) in the pivot column: the ONE fused update c <- c - m re of another row then leaves
                        // m - m (1 + 1/p) = -m / p there -- the multiplier the in-place inverse keeps in that column -- with no blend per row (two v_cndmask and a
                        // multiply per row and pivot were half of the elimination's instructions).  Error of that entry: |m| (1 + |1/p|) ulp, i.e. relative
                        // (1 + |p|) ulp -- p is the largest entry of its row.
                        const double re = isj ? 1.0 + inv : rv * inv;
                        NS_PACC(1);
                        static_for<NR1 / 8>([&](auto gc) {
                            constexpr int g = decltype(gc)::value;
                            if (8 * g < neq) {          // (uniform; one test per eight rows)
                                double ml[8];
                                static_for<8>([&](auto kc) {          // the eight multipliers first (v_readlane pairs back to back), then the eight updates
                                    constexpr int i = 8 * g + decltype(kc)::value;
                                    ml[decltype(kc)::value] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(c1[i]), jb), __builtin_amdgcn_readlane(__double2loint(c1[i]), jb));
                                });
                                static_for<8>([&](auto kc) {
                                    constexpr int i = 8 * g + decltype(kc)::value;
                                    if constexpr (i != e) c1[i] = fma(-ml[decltype(kc)::value], re, c1[i]);          // (the pivot column keeps the multiplier -> column e of B_1^-1)
                                });
                            }
                        });
                        c1[e] = isj ? inv : re;          // (the pivot row itself: 1/p in the pivot column)
                        cfr = cfr && !isj;
                        if (lane == 0) pcol[e] = jb;
                        NS_PACC(2);
                    } else if (lane == 0) { pcol[e] = -1; misc[2] |= 4; }          // redundant equality row: dropped (mu_e = 0), the instance is flagged
                }
            });
            static_for<NR1>([&](auto kc) {
                constexpr int kk = decltype(kc)::value;
                if (kk < neq) { double *ptr = sm + erow[kk]; if (lane < n) ptr[lane] = c1[kk]; else if (lane == n) dB[kk] = c1[kk]; }
            });
            const bool fr = lane < n && cfr;
            const unsigned long long bal = __ballot(fr);
            if (lane < n) { if (fr) { const int f = __popcll(bal & ((1ull << lane) - 1ull)); cmap[lane] = f; fcol[f] = lane; } else cmap[lane] = -1; }
            if (lane == 0) misc[1] = __popcll(bal);
#ifdef CE_TIMING
            if (lane == 0) for (int k = 0; k < 4; k++) tsub[8 + k] = pacc[k];
#endif
        }
    } else {
        double col[NLOC][NSL];
        double rtol[NLOC];          // rank tolerance of a row: CE_RANK_TOL x its largest entry as loaded (scale-invariant per row; a redundant row ends at rounding level of that)
        bool cfree[NSL];
        static_for<NLOC>([&](auto kc) {          // (a compile-time loop: a plain unroll of this body stayed rolled and put the rows in scratch)
            constexpr int kk = decltype(kc)::value;
            const int e = wave + NWB * kk;
            const double *ptr = sm + (e < neq ? erow[e] : 0);
            const double de = e < neq ? dB[e] : 0.0;
            double rmax = 0.0;
#pragma unroll
            for (int s2 = 0; s2 < NSL; s2++) {
                const int j = lane + 64 * s2;
                const double v = (e < neq && j < n) ? ptr[j < n ? j : 0] : 0.0;
                rmax = fmax(rmax, fabs(v));
                col[kk][s2] = (e < neq && j == n) ? de : v;
            }
            rmax = wave_reduce_dpp<true>(rmax);
            rtol[kk] = CE_RANK_TOL * (rmax > 0 ? rmax : 1.0);
        });
#pragma unroll
        for (int s2 = 0; s2 < NSL; s2++) cfree[s2] = true;
        for (int e = 0; e < neq; e++) {
            const int wo = e % NWB, k = e / NWB;
            double *pb = pub + (e & 1) * PUBP;
            if (wave == wo) {
                double re[NSL], ptolB = 0.0;
#pragma unroll
                for (int s2 = 0; s2 < NSL; s2++) re[s2] = 0.0;
                static_for<NLOC>([&](auto kc) {
                    constexpr int kk = decltype(kc)::value;
                    if (k == kk) {
#pragma unroll
                        for (int s2 = 0; s2 < NSL; s2++) re[s2] = col[kk][s2];
                        ptolB = rtol[kk];
                    }
                });
                double best = 0.0;
#pragma unroll
                for (int s2 = 0; s2 < NSL; s2++) {
                    const int j = lane + 64 * s2;
                    const double key = __hiloint2double(__double2hiint(re[s2]) & 0x7fffffff, (__double2loint(re[s2]) & ~0xFF) | (255 - j));      // |value|, 255 - column in the low mantissa bits
                    best = fmax(best, (j < n && cfree[s2]) ? key : 0.0);
                }
                best = wave_reduce_dpp<true>(best);
                const int jb = 255 - (__double2loint(best) & 0xFF);
                const bool ok = best >= ptolB && jb < n;
                const int jl = ok ? (jb & 63) : 0;
                double pv = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(re[0]), jl), __builtin_amdgcn_readlane(__double2loint(re[0]), jl));
                if constexpr (NSL > 1) { if (jb >= 64) pv = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(re[NSL - 1]), jl), __builtin_amdgcn_readlane(__double2loint(re[NSL - 1]), jl)); }
                const double pvs = ok ? pv : 1.0;
                double inv = __builtin_amdgcn_rcp(pvs);          // hardware seed + two Newton steps (the IEEE divide expansion sits on the path every wave waits for)
                inv = fma(fma(-pvs, inv, 1.0), inv, inv);
                inv = fma(fma(-pvs, inv, 1.0), inv, inv);
                inv = ok ? inv : 0.0;
#pragma unroll
                for (int s2 = 0; s2 < NSL; s2++) pb[lane + 64 * s2] = (lane + 64 * s2 == jb) ? 1.0 + inv : re[s2] * inv;      // (1 + 1/p in the pivot column: see the single-wave path)
                if (lane == 0) {
                    pb[NCOLP] = inv; reinterpret_cast<int *>(pb + NCOLP + 1)[0] = ok ? jb : -1;
                    pcol[e] = ok ? jb : -1;
                    if (!ok) misc[2] |= 4;          // redundant equality row: dropped (mu_e = 0), the instance is flagged
                }
            }
            __syncthreads();
            // header, inverse pivot and this lane's entries of the scaled row in ONE round trip (requested together, before the header is looked at)
            const int jbv = reinterpret_cast<const int *>(pb + NCOLP + 1)[0];
            const double inv = pb[NCOLP];
            double r[NSL];
#pragma unroll
            for (int s2 = 0; s2 < NSL; s2++) r[s2] = pb[lane + 64 * s2];
            const int jb = __builtin_amdgcn_readfirstlane(jbv);
            if (jb < 0) continue;
            const int jl = jb & 63;
            static_for<(NLOC + 3) / 4>([&](auto gc) {
                constexpr int g = decltype(gc)::value;
                if (NWB * 4 * g < neq) {          // (uniform; one test per four local rows: rows past neq hold zeros and are harmless to update)
                    static_for<4>([&](auto kc) {
                        constexpr int kk = 4 * g + decltype(kc)::value;
                        if constexpr (kk < NLOC) {
                            const int ei = wave + NWB * kk;
                            double mlt = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(col[kk][0]), jl), __builtin_amdgcn_readlane(__double2loint(col[kk][0]), jl));
                            if constexpr (NSL > 1) { if (jb >= 64) mlt = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(col[kk][NSL - 1]), jl), __builtin_amdgcn_readlane(__double2loint(col[kk][NSL - 1]), jl)); }
                            const bool isp = ei == e;          // (uniform: the pivot row itself becomes the scaled row, 1/p in the pivot column)
#pragma unroll
                            for (int s2 = 0; s2 < NSL; s2++) {
                                const int j = lane + 64 * s2;
                                col[kk][s2] = isp ? ((j == jb) ? inv : r[s2]) : fma(-mlt, r[s2], col[kk][s2]);          // the pivot column keeps the multiplier (-> column e of B_1^-1)
                            }
                        }
                    });
                }
            });
#pragma unroll
            for (int s2 = 0; s2 < NSL; s2++) if (lane + 64 * s2 == jb) cfree[s2] = false;
        }
        // rows back to LDS (in place: R in the free columns, B_1^-1 in the pivot columns), d~ -> dB
        static_for<NLOC>([&](auto kc) {
            constexpr int kk = decltype(kc)::value;
            const int e = wave + NWB * kk;
            if (e < neq) {
                double *ptr = sm + erow[e];
#pragma unroll
                for (int s2 = 0; s2 < NSL; s2++) { const int j = lane + 64 * s2; if (j < n) ptr[j] = col[kk][s2]; else if (j == n) dB[e] = col[kk][s2]; }
            }
        });
        if (wave == 0) {          // free columns numbered in increasing order (cfree is the same in every wave)
            int basef = 0;
#pragma unroll
            for (int s2 = 0; s2 < NSL; s2++) {
                const int j = lane + 64 * s2;
                const bool fr = j < n && cfree[s2];
                const unsigned long long bal = __ballot(fr);
                if (j < n) {
                    if (fr) { const int f = basef + __popcll(bal & ((1ull << lane) - 1ull)); cmap[j] = f; fcol[f] = j; }
                    else cmap[j] = -1;
                }
                basef += __popcll(bal);
            }
            if (lane == 0) misc[1] = basef;
        }
    }
    __syncthreads();
    NS_STAMP(4);
    if constexpr (QP) { for (int e = tid; e < neq; e += NTHR) { const int pc = pcol[e]; if (pc >= 0) peq[pc] = e; } }          // (read behind the barrier that ends step 2)
    const int nf = misc[1];
    const int NB = (nf + 3) >> 2, cr = 4 * NB;          // blocks of four that hold a reduced variable; column of the right-hand side
    // ---- 2. null-space transform of the weighted rows and of f (list entry KW), in place, on the matrix cores:
    //      row[j] <- row[j] - sum_e row[p_e] R[e][j]  (free j),   t = sum_e row[p_e] d~_e        i.e.  D = A_w[:, piv] [R | d~]   (KW+1 x neq) (neq x n+1)
    //      wave J owns the column tile 16 J .. 16 J + 15 (column n = t); 64 list rows per pass; K = the equalities, four per instruction.
    {
        const int NCT = (n + 16) >> 4;                   // column tiles that hold a column <= n
        if (wave < NCT) {
            const int colj = 16 * wave + lc;
            for (int g0 = 0; g0 <= KW; g0 += 64) {
                const int ng = min(4, (KW - g0 + 16) >> 4);          // row groups of this pass that hold a list row <= KW (uniform)
                v4d tacc[4];
                int wr[4];
#pragma unroll
                for (int g = 0; g < 4; g++) { tacc[g] = v4d{0.0, 0.0, 0.0, 0.0}; wr[g] = wrow[min(g0 + 16 * g + lc, KW4 - 1)]; }
                for (int k0 = 0; k0 < neq; k0 += 4) {
                    const int kq = min(k0 + lg, neq - 1);
                    const int pc = (k0 + lg < neq) ? pcol[kq] : -1, er = erow[kq];
                    const double bop = (pc >= 0 && colj <= n) ? (colj < n ? sm[er + colj] : dB[kq]) : 0.0;
                    const int pcs = pc >= 0 ? pc : 0;
                    double aop[4];
#pragma unroll
                    for (int g = 0; g < 4; g++) aop[g] = sm[wr[g] + pcs];
#pragma unroll
                    for (int g = 0; g < 4; g++) if (g < ng) tacc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(pc >= 0 ? aop[g] : 0.0, bop, tacc[g], 0, 0, 0);
                }
                // write-back in three fenced stages (list offsets, old values, stores): sixteen dependent read-modify-writes in series otherwise
                const bool wcol = colj < n && cmap[colj < n ? colj : 0] >= 0, tcol = colj == n;
                int wq[4][4];
#pragma unroll
                for (int g = 0; g < 4; g++)
#pragma unroll
                    for (int r = 0; r < 4; r++) wq[g][r] = wrow[min(g0 + 16 * g + lg + 4 * r, KW4 - 1)];
                __builtin_amdgcn_sched_barrier(0);
                double ov[4][4];
                const int cj = colj < n ? colj : 0;
#pragma unroll
                for (int g = 0; g < 4; g++)
#pragma unroll
                    for (int r = 0; r < 4; r++) ov[g][r] = sm[wq[g][r] + cj];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int g = 0; g < 4; g++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int q = g0 + 16 * g + lg + 4 * r;
                        if (q <= KW) {
                            if (wcol) sm[wq[g][r] + cj] = ov[g][r] - tacc[g][r];
                            else if (tcol && q < KW) tvec[q] = tacc[g][r];
                        }
                    }
            }
        }
        if constexpr (QP) {
            // the rows of P through the same transform, sixteen per pass:  p_j[free] <- p_j[free] - sum_e p_j[p_e] R[e][free],  t_j = sum_e p_j[p_e] d~_e -> ptv.
            // The pivot columns of P are only read here and stay as loaded (the multipliers need them).
            if (wave < NCT) {
                const int colj = 16 * wave + lc, cj = colj < n ? colj : 0;
                const bool wcol = colj < n && cmap[cj] >= 0, tcol = colj == n;
                for (int g0 = 0; g0 < n; g0 += 16) {
                    v4d tacc = v4d{0.0, 0.0, 0.0, 0.0};
                    const int prw = min(g0 + lc, n - 1) * n;
                    for (int k0 = 0; k0 < neq; k0 += 4) {
                        const int kq = min(k0 + lg, neq - 1);
                        const int pc = (k0 + lg < neq) ? pcol[kq] : -1, er = erow[kq];
                        const double bop = (pc >= 0 && colj <= n) ? (colj < n ? sm[er + colj] : dB[kq]) : 0.0;
                        const double aop = Pm[prw + (pc >= 0 ? pc : 0)];
                        tacc = __builtin_amdgcn_mfma_f64_16x16x4f64(pc >= 0 ? aop : 0.0, bop, tacc, 0, 0, 0);
                    }
                    static_for<4>([&](auto rc) {
                        constexpr int r = decltype(rc)::value;
                        const int q = g0 + lg + 4 * r;
                        if (q < n) { if (wcol) Pm[q * n + cj] -= tacc[r]; else if (tcol) ptv[q] = tacc[r]; }
                    });
                }
            }
        }
    }
    __syncthreads();
    NS_STAMP(5);
    // ---- 3. reduced Hessian (+ right-hand side as column cr) on the matrix cores: wave w accumulates the strip of rows 16 w .. 16 w + 15.
    //      Operands two steps ahead of the instruction that consumes them (list entry, then the row's values): the loop is a chain of LDS round trips otherwise.
    v4d acc[NTILE];
#pragma unroll
    for (int J = 0; J < NTILE; J++) acc[J] = v4d{0.0, 0.0, 0.0, 0.0};
    const int jmax = (cr >> 4) + 1;                     // tiles / strips that hold a row or column <= cr
    if (wave < jmax) {
        // Operand addresses, not operand arithmetic: a lane whose reduced column does not exist reads a ZERO (a pad entry of tvec), the lane of the right-hand-side
        // column reads t_q itself (the column is negated behind the loop), every other lane reads the row's entry of its original column -- so the B operands go
        // from LDS straight into the matrix cores and the A operand takes ONE multiply (the weight).  With fp64 multiplies and blends between the MFMAs the loop
        // ran at ~200 cycles per MFMA (the fp64 vector operations queue behind the matrix instruction in flight); requested in batches of four steps.
        const int tvoff = (int)(tvec - sm), zoff = tvoff + KW;          // (tvec[KW] is a pad entry: 0.0)
        int oc[NTILE], kd[NTILE];          // per tile: original column of this lane's reduced column; kind 0 row entry, 1 the step's t_q, 2 zero
#pragma unroll
        for (int J = 0; J < NTILE; J++) {
            const int colr = 16 * J + lc;
            oc[J] = colr < nf ? fcol[colr < nf ? colr : 0] : 0; kd[J] = colr < nf ? 0 : (colr == cr ? 1 : 2);
        }
        int ocw = 0, kdw = 2;
        static_for<NTILE>([&](auto Jc) { constexpr int J = decltype(Jc)::value; if (wave == J) { ocw = oc[J]; kdw = kd[J]; } });
        double frhs[4];          // (Z^T f)[row] of this lane's four strip rows: requested now, used behind the loop
#pragma unroll
        for (int r = 0; r < 4; r++) { const int rowi = 16 * wave + lg + 4 * r; frhs[r] = fvec[fcol[rowi < nf ? rowi : 0]]; }
        NS_SUB(0);
        constexpr int UB = 4;
        int wr[UB]; double ww[UB];
#pragma unroll
        for (int u = 0; u < UB; u++) { const int q = min(4 * u + lg, KW4 - 1); wr[u] = wrow[q]; ww[u] = wgt[q]; }
        for (int k0 = 0; k0 < KW4; k0 += 4 * UB) {
            double aB[UB], bB[UB][NTILE];
#pragma unroll
            for (int u = 0; u < UB; u++) {
                const int tq = tvoff + min(k0 + 4 * u + lg, KW4 - 1);
                aB[u] = sm[kdw == 0 ? wr[u] + ocw : (kdw == 1 ? tq : zoff)];
#pragma unroll
                for (int J = 0; J < NTILE; J++) bB[u][J] = sm[kd[J] == 0 ? wr[u] + oc[J] : (kd[J] == 1 ? tq : zoff)];
            }
            double wc[UB];
#pragma unroll
            for (int u = 0; u < UB; u++) wc[u] = ww[u];
#pragma unroll
            for (int u = 0; u < UB; u++) { const int q = min(k0 + 4 * UB + 4 * u + lg, KW4 - 1); wr[u] = wrow[q]; ww[u] = wgt[q]; }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < UB; u++) aB[u] *= wc[u];          // the four weighted A operands first, then nothing but matrix instructions
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < UB; u++) {
                if (k0 + 4 * u < KW4) {          // (uniform: the last batch may be short)
#pragma unroll
                    for (int J = 0; J < NTILE; J++) if (J < jmax) acc[J] = __builtin_amdgcn_mfma_f64_16x16x4f64(aB[u], bB[u][J], acc[J], 0, 0, 0);
                }
            }
        }
        if constexpr (QP) {
            // + Z^T P Z = sum_j z_j p~_j^T over the n rows of P, four per instruction: the A operand is z_j at this lane's strip row (1 at the free column j itself,
            // -R[e][.] for the pivot column of equality e), the B operands are p~_j at the tile's columns and t_j in the right-hand-side column (+ Z^T P x_p there:
            // the column is negated below).  Formed by value, not by address: one run of n / 4 steps beside the KW / 4 of the loop above.
            const int frow = 16 * wave + lc;
            for (int k0 = 0; k0 < n; k0 += 4) {
                const bool jv = k0 + lg < n;
                const int j = jv ? k0 + lg : n - 1;
                const int cm = cmap[j];
                double za = 0.0;
                if (jv && kdw == 0) { if (cm >= 0) za = cm == frow ? 1.0 : 0.0; else za = -sm[erow[peq[j]] + ocw]; }
                const double tj = ptv[j];
                double bP[NTILE];
#pragma unroll
                for (int J = 0; J < NTILE; J++) { const double pv = Pm[j * n + oc[J]]; bP[J] = kd[J] == 0 ? pv : (kd[J] == 1 ? tj : 0.0); }
#pragma unroll
                for (int J = 0; J < NTILE; J++) if (J < jmax) acc[J] = __builtin_amdgcn_mfma_f64_16x16x4f64(za, bP[J], acc[J], 0, 0, 0);
            }
        }
        NS_SUB(1);
        // + Z^T f on the right-hand-side column; identity on the padding rows of the last block
        static_for<NTILE>([&](auto Jc) {
            constexpr int J = decltype(Jc)::value;
            static_for<4>([&](auto rc) {          // (compile-time indices into the accumulators: a rolled loop here puts them in scratch)
                constexpr int r = decltype(rc)::value;
                const int rowi = 16 * wave + lg + 4 * r;
                const bool rhs = 16 * J + lc == cr;          // the right-hand-side column: Z^T f - sum_k w_k t_k a~_k (the loop accumulated + sum w t a~ there)
                const bool pad = wave == J && lc == lg + 4 * r && rowi >= nf && rowi < cr;
                acc[J][r] = pad ? 1.0 : (rhs ? (rowi < nf ? frhs[r] : 0.0) - acc[J][r] : acc[J][r]);
            });
        });
    }
    NS_SUB(2);
    __syncthreads();          // the Gram's reads of a_z are complete: the union region becomes the sweep's row buffers
    // the ORIGINAL diagonal of the reduced Hessian -> the gaps behind the buffer rows (entry k at row k >> 4 of the buffers, 16 NTILE + (k & 15)); rows 0 .. 3 -> buffer 0
    if (wave < NTILE) {
        static_for<NTILE>([&](auto Jc) {
            constexpr int J = decltype(Jc)::value;
            if (wave == J) {
                double dsel = 0.0;
                static_for<4>([&](auto rc) { constexpr int r = decltype(rc)::value; dsel = (lc == lg + 4 * r) ? acc[J][r] : dsel; });
                if ((lc & 3) == lg) Rbuf[J * LDP + 16 * NTILE + lc] = dsel;          // (the diagonal lanes: lc = lg + 4 r)
            }
        });
    }
    NS_STAMP(6);
    // ---- 4. blocked sweep on the matrix cores (ce_forward_v2.h, S inversion): after block b the rows K = {4b .. 4b+3} hold P R, the others S - C P R;
    //      the right-hand-side column ends as (Z^T H Z)^-1 rhs.  A pivot that is not positive against the tolerance drops its variable (pivot inverse 0) and flags.
    if (wave == 0) {
#pragma unroll
        for (int J = 0; J < NTILE; J++) Rbuf[lg * LDP + 16 * J + lc] = acc[J][0];
    }
    __syncthreads();
    bool tiny = false;
    static_for<4 * NTILE>([&](auto bc) {
        constexpr int b = decltype(bc)::value, k0 = 4 * b, wo = k0 / 16, r0 = (k0 % 16) / 4, c0 = k0 % 16;
        constexpr int k1 = k0 + 4, wn = (k1 / 16) % NTILE, r1 = (k1 % 16) / 4;
        if (b < NB) {
            const double *Rb = Rbuf + (b & 1) * (4 * LDP);
            double *Rn = Rbuf + ((b + 1) & 1) * (4 * LDP);
            if (wave < NTILE) {
                double Bop[NTILE], Cop[4], a[4][4];
#pragma unroll
                for (int J = 0; J < NTILE; J++) Bop[J] = Rb[lg * LDP + 16 * J + lc];
                {
                    int coff = 16 * wave + lc;
                    asm volatile("" : "+v"(coff));
#pragma unroll
                    for (int pq = 0; pq < 4; pq++) Cop[pq] = Rb[pq * LDP + coff];
                }
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const double2 v0 = *reinterpret_cast<const double2 *>(Rb + q * LDP + k0), v1 = *reinterpret_cast<const double2 *>(Rb + q * LDP + k0 + 2);
                    a[q][0] = v0.x; a[q][1] = v0.y; a[q][2] = v1.x; a[q][3] = v1.y;
                }
                double dg[4];          // the block's original diagonal entries (rank tolerance relative to each)
                {
                    const double2 d0 = *reinterpret_cast<const double2 *>(Rbuf + wo * LDP + 16 * NTILE + c0), d1 = *reinterpret_cast<const double2 *>(Rbuf + wo * LDP + 16 * NTILE + c0 + 2);
                    dg[0] = d0.x; dg[1] = d0.y; dg[2] = d1.x; dg[3] = d1.y;
                }
                __builtin_amdgcn_sched_barrier(0);
                double e[4];
#pragma unroll
                for (int k = 0; k < 4; k++) e[k] = (lg == k) ? 1.0 : 0.0;
                double pinv[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double pv = a[k][k];
                    const bool ok = pv > CE_RANK_TOL * dg[k];
                    tiny |= !ok;
                    const double pvs = ok ? pv : 1.0;
                    double pi_ = __builtin_amdgcn_rcp(pvs);
                    pi_ = fma(fma(-pvs, pi_, 1.0), pi_, pi_);
                    pi_ = fma(fma(-pvs, pi_, 1.0), pi_, pi_);
                    pi_ = ok ? pi_ : 0.0;
                    pinv[k] = pi_;
#pragma unroll
                    for (int i = k + 1; i < 4; i++) {
                        const double lm = a[i][k] * pi_;
#pragma unroll
                        for (int j = k + 1; j < 4; j++) a[i][j] = fma(-lm, a[k][j], a[i][j]);
                        e[i] = fma(-lm, e[k], e[i]);
                    }
                }
                double xs[4];
                xs[3] = e[3] * pinv[3];
                xs[2] = fma(-a[2][3], xs[3], e[2]) * pinv[2];
                xs[1] = fma(-a[1][3], xs[3], fma(-a[1][2], xs[2], e[1])) * pinv[1];
                xs[0] = fma(-a[0][3], xs[3], fma(-a[0][2], xs[2], fma(-a[0][1], xs[1], e[0]))) * pinv[0];
                double wsel = -(Cop[0] * xs[0] + Cop[1] * xs[1] + Cop[2] * xs[2] + Cop[3] * xs[3]);
                const int mr = lc - c0;
                const bool kcol = mr >= 0 && mr < 4;
                const double nk = kcol ? 0.0 : 1.0;
                if (wave == wo) {
                    double psel = 0.0;
#pragma unroll
                    for (int k = 0; k < 4; k++) psel = fma(xs[k], (mr == k) ? 1.0 : 0.0, psel);
                    wsel = fma(wsel, nk, psel);
#pragma unroll
                    for (int J = 0; J < NTILE; J++) acc[J][r0] = 0.0;
                }
#pragma unroll
                for (int r = 0; r < 4; r++) acc[wo][r] *= nk;
                Bop[wo] = fma(Bop[wo], nk, (kcol && mr == lg) ? -1.0 : 0.0);
#pragma unroll
                for (int J = 0; J < NTILE; J++) acc[J] = __builtin_amdgcn_mfma_f64_16x16x4f64(wsel, Bop[J], acc[J], 0, 0, 0);
                if (b + 1 < NB && wave == wn) {
#pragma unroll
                    for (int J = 0; J < NTILE; J++) Rn[lg * LDP + 16 * J + lc] = acc[J][r1];
                }
            }
            __syncthreads();
        }
    });
    if (tiny && lane == 0) misc[2] |= 4;          // (every lane of every strip solved the same 4 x 4 blocks: the flag is uniform)
    NS_STAMP(7);
    // ---- MANY: steps 1-4 ran on a zero right-hand side.  The sweep is an in-place inversion: the accumulator tiles hold -(Z^T H Z)^-1, the pivot columns of the
    //      eliminated rows B_1^-1, their free columns R, the list rows a~ in the free columns and a in the pivot columns.  Everything a cotangent touches is rebuilt
    //      from those, one cotangent after the other, and step 5 and the epilogue run per cotangent on the same buffers.
    int nrhs = 1;
    if constexpr (MANY) nrhs = W.K;
    for (int kc = 0; kc < nrhs; kc++) {
    const double *dxk = dxg, *dyk = dyg;
    double *dAk = dAo, *dqk = dqo;
    int *adjk = adj_status;
    if constexpr (MANY && FWD) {
        // ---- K tangents: what the forward prologue, the classification pass and the passes in front of step 1 leave in the buffers, rebuilt for tangent kc from the
        //      retained state (rkind, ckind, cinfo's lambda, |z| and theta, eqrow / ceq, the in-place inverses, the list rows).  x and y come from global memory again (y
        //      waits in tvec, x in rx, as in the single-tangent load): the tangent products need the tangent's values and the point, not A, which is transformed by now.
        if (adjk) adjk += kc * W.sak;
        const double *const tAk = W.tA ? W.tA + kc * W.stAk + (size_t)inst * W.stAb : nullptr;          // (stAb == 0: one tangent row for the whole batch; tq, tP alike)
        const double *const tqk = W.tq ? W.tq + kc * W.stqk + (size_t)inst * W.stqb : nullptr;
        const double *tPk = nullptr;
        if constexpr (QP) tPk = W.Q.tP ? W.Q.tP + kc * W.stPk + (size_t)inst * W.stPb : nullptr;
        __syncthreads();          // the output pass of the tangent before has read vv, rx and dv
        for (int i = tid; i < m; i += NTHR) { const double yi = yg[(size_t)inst * m + i]; vv[i] = yi - sg[(size_t)inst * m + i]; tvec[i] = yi; }
        for (int j = tid; j < n; j += NTHR) rx[j] = xg[(size_t)inst * n + j];
        __syncthreads();
        fwd_prologue(tAk, tqk, 1, tPk);          // g_x -> fvec, g_y -> dv (dv keeps it unrotated up to the epilogue)
        __syncthreads();
        // per boundary cone gamma_y, gamma_s and the weights u_i = theta (g_i - z-hat_i (z-hat . g_z)) of its z-rows, from the retained lambda, |z|, theta; the weights
        // wait in qv2 BY ROW (the union region is free behind the sweep; tvec is the list's).  The t-row has weight 0: f has no a_y share here.
        for (int c0 = 0; c0 < nq; c0 += NTHR / 16) {
            const int c = c0 + (tid >> 4), l16 = tid & 15;
            const bool cv = c < nq && ckind[c < nq ? c : 0] == 2;
            const int r0 = cv ? T.qoff[c] : 0, r1 = cv ? T.qoff[c + 1] : 0;
            const double h0 = cv ? dv[r0] : 0.0, nz = cv ? cinfo[5 * c + 1] : 1.0, th = cv ? cinfo[5 * c + 4] : 0.0;
            double zh = 0.0;
            for (int i = r0 + 1 + l16; i < r1; i += 16) zh = fma(vv[i], dv[i], zh);
            zh = group_reduce<16, false>(zh);
            const double zeta = zh / nz, inz = 1.0 / nz;
            for (int i = r0 + 1 + l16; i < r1; i += 16) qv2[i] = th * (dv[i] - vv[i] * inz * zeta);
            if (cv && l16 == 0) { cinfo[5 * c + 2] = (h0 + zeta) * M_SQRT1_2; cinfo[5 * c + 3] = (h0 - zeta) * M_SQRT1_2; }
        }
        if constexpr (TRI) {
            // triples, one thread per triple, from the retained W and lambda: the rows keep gamma = W^T g_y (a lambda = 1 row: its entry of d_B, taken by eqrow below; a
            // lambda = 0 row: nothing in f, the epilogue wants its gamma), and a weighted row's share of f, theta gamma, waits in qv2 BY ROW beside the boundary cones'
            for (int c = tid; c < ntri; c += NTHR) {
                const int r0 = T.eoff + 3 * c;
                const double *Wl = Wt + 9 * c;
                const double h0 = dv[r0], h1 = dv[r0 + 1], h2 = dv[r0 + 2];
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    const double t = Wl[a] * h0 + Wl[3 + a] * h1 + Wl[6 + a] * h2, lam = lamt[3 * c + a];
                    dv[r0 + a] = t;
                    qv2[r0 + a] = rkind[r0 + a] == RK_MIX ? lam / (1 - lam) * t : 0.0;
                }
            }
        }
        if constexpr (PSD && MANY) {
            // PSD blocks, from the retained U and B: the rows keep gamma_c = Q^T g_y,c (a B = 1 row: its entry of d_B, taken by eqrow below; a B = 0 row: nothing in f, the
            // epilogue wants its gamma), and a weighted row's share of f, theta gamma, waits in qv2 BY ROW beside the boundary cones'
            __syncthreads();
            psd_rotate_vec(dv, false);
            for (int i = psd0 + tid; i < T.eoff; i += NTHR) { const double lam = lamp[i - psd0]; qv2[i] = rkind[i] == RK_MIX ? lam / (1 - lam) * dv[i] : 0.0; }
        }
        __syncthreads();
        // d_B = gamma_B by equality (eqrow and ceq are the numbering's inverse) -> mu
        for (int i = tid; i < m; i += NTHR) if (rkind[i] == RK_EQ) mu[eqrow[i]] = dv[i];
        for (int c = tid; c < nq; c += NTHR) if (ckind[c] == 2) mu[ceq[c]] = cinfo[5 * c + 2];
        __syncthreads();
        // d~ = B_1^-1 d_B from the in-place inverse: 16 lanes per equality
        for (int e0 = 0; e0 < neq; e0 += NTHR / 16) {
            const int e = e0 + (tid >> 4), part = tid & 15;
            double a = 0.0;
            const int pc = e < neq ? pcol[e] : -1;
            if (pc >= 0) { const double *row = sm + erow[e]; for (int i = part; i < neq; i += 16) { const int pi = pcol[i]; if (pi >= 0) a = fma(row[pi], mu[i], a); } }
            a = group_reduce<16, false>(a);
            if (e < neq && part == 0) dB[e] = pc >= 0 ? a : 0.0;
        }
        __syncthreads();
        // t_q = a_q . x_p for the z-rows of the list (their pivot columns are as loaded); QP: t_j = p_j . x_p for the rows of P (its pivot columns are untouched) -> ptv
        auto list_t = [&]() {
            for (int q0 = 0; q0 < KW; q0 += NTHR / 4) {
                const int q = q0 + (tid >> 2), part = tid & 3;
                const bool live = q < KW && wsrc[q < KW ? q : 0] >= 0;
                double a = 0.0;
                if (live) { const double *row = sm + wrow[q]; for (int e = part; e < neq; e += 4) { const int pc = pcol[e]; if (pc >= 0) a = fma(row[pc], dB[e], a); } }
                a = group_reduce<4, false>(a);
                if (live && part == 0) tvec[q] = a;
            }
        };
        list_t();
        if constexpr (QP) {
            for (int j0 = 0; j0 < n; j0 += NTHR / 4) {
                const int j = j0 + (tid >> 2), part = tid & 3;
                double a = 0.0;
                if (j < n) for (int e = part; e < neq; e += 4) { const int pc = pcol[e]; if (pc >= 0) a = fma(Pm[j * n + pc], dB[e], a); }
                a = group_reduce<4, false>(a);
                if (j < n && part == 0) ptv[j] = a;
            }
        }
        __syncthreads();
        // the list takes theta q'_i = theta (t_i - z-hat_i (z-hat . t)): Z^T H x_p = sum theta q'_i a~_i needs no a_z (whose storage was the sweep's)
        for (int c = tid; c < nq; c += NTHR) {
            if (ckind[c] != 2) continue;
            const int r0 = T.qoff[c], r1 = T.qoff[c + 1], qb = cbase[c];
            const double inz = 1.0 / cinfo[5 * c + 1], th = cinfo[5 * c + 4];
            double zt = 0.0;
            for (int i = r0 + 1; i < r1; i++) zt = fma(vv[i], tvec[qb + i - r0 - 1], zt);
            zt *= inz;
            for (int i = r0 + 1; i < r1; i++) { const double zhi = vv[i] * inz; tvec[qb + i - r0 - 1] = th * (tvec[qb + i - r0 - 1] - zhi * zt); }
        }
        if constexpr (TRI) {          // a triple's weighted row is one list row of its own: theta t (eqrow keeps its list entry)
            for (int i = T.eoff + tid; i < m; i += NTHR) if (rkind[i] == RK_MIX) { const int q = eqrow[i]; tvec[q] *= wgt[q]; }
        }
        if constexpr (PSD && MANY) {          // so is a block's weighted row
            for (int i = psd0 + tid; i < T.eoff; i += NTHR) if (rkind[i] == RK_MIX) { const int q = eqrow[i]; tvec[q] *= wgt[q]; }
        }
        __syncthreads();
        // f = -g_x + sum u_i a_i by column.  A pivot column keeps f[piv] (the multipliers want it); a free column takes  h + sum (u_i - theta q'_i) a~_i  with
        // h = -g_x [- P x_p], which lacks only -R^T h[piv] of the reduced right-hand side Z^T (f - (H [+ P]) x_p).  h waits in rx.  4 lanes per column, fixed order.
        for (int j0 = 0; j0 < n; j0 += NTHR / 4) {
            const int j = j0 + (tid >> 2), part = tid & 3;
            double a = 0.0, b = 0.0;
            if (j < n) for (int q = part; q < KW; q += 4) {
                const int ws = wsrc[q];
                if (ws >= 0) { const double av = sm[wrow[q] + j]; a = fma(av, qv2[ws], a); b = fma(av, tvec[q], b); }
            }
            a = group_reduce<4, false>(a); b = group_reduce<4, false>(b);
            if (j < n && part == 0) {
                const double gx = fvec[j];
                double hj = -gx;
                if constexpr (QP) hj -= ptv[j];
                rx[j] = hj;
                fvec[j] = cmap[j] >= 0 ? hj + a - b : a - gx;
            }
        }
        __syncthreads();
        list_t();          // (tvec holds t again: step 5 adds a~ . x_free to it)
        for (int j = tid; j < n; j += NTHR) {
            if (cmap[j] < 0) continue;
            double a = fvec[j];
            for (int e = 0; e < neq; e++) { const int pc = pcol[e]; if (pc >= 0) a = fma(-sm[erow[e] + j], rx[pc], a); }
            fvec[j] = a;
        }
        __syncthreads();
        for (int j = tid; j < n; j += NTHR) rx[j] = 0.0;          // (step 5 wants zeros in the pivot entries; the free ones are written next)
        __syncthreads();
        // x_free = (Z^T (H [+ P]) Z)^-1 rhs out of the accumulator tiles, as the many-cotangent adjoint takes it
        if (wave < NTILE) {
            double rr[NTILE];
#pragma unroll
            for (int J = 0; J < NTILE; J++) { const int colr = 16 * J + lc; rr[J] = colr < nf ? fvec[fcol[colr < nf ? colr : 0]] : 0.0; }
            static_for<4>([&](auto rc) {
                constexpr int r = decltype(rc)::value;
                double sacc = 0.0;
                static_for<NTILE>([&](auto Jc) { constexpr int J = decltype(Jc)::value; sacc = fma(acc[J][r], rr[J], sacc); });
                sacc = group_reduce<16, false>(sacc);
                const int rowi = 16 * wave + lg + 4 * r;
                if (lc == 0 && rowi < nf) rx[fcol[rowi]] = -sacc;
            });
        }
    } else if constexpr (MANY) {
        dxk += kc * W.sxk; dyk += kc * W.syk; dAk += kc * W.sAk; dqk += kc * W.sqk; if (adjk) adjk += kc * W.sak;
        const double *const dxi = dxk + (size_t)inst * n;
        __syncthreads();          // the output pass of the cotangent before has read vv, rx, fvec and dv
        for (int i = tid; i < m; i += NTHR) { vv[i] = yg[(size_t)inst * m + i] - sg[(size_t)inst * m + i]; dv[i] = dyk[(size_t)inst * m + i]; }
        for (int j = tid; j < n; j += NTHR) rx[j] = 0.0;
        __syncthreads();
        // d = DPi(v) dy and the per-cone scalars from the retained classification (ckind, lambda, |z|); the weights u of f = dx + A^T u wait in qv2 BY ROW (the
        // union region is free behind the sweep; tvec is the list's)
        for (int i = tid; i < z + T.l; i += NTHR) if (rkind[i] != RK_EQ) dv[i] = 0.0;
        for (int c0 = 0; c0 < nq; c0 += NTHR / 16) {
            const int c = c0 + (tid >> 4), l16 = tid & 15;
            const bool cv = c < nq;
            const int r0 = cv ? T.qoff[c] : 0, r1 = cv ? T.qoff[c + 1] : 0;
            const int kind = cv ? ckind[c] : 0;
            const double lam = cv ? cinfo[5 * c] : 0.0, nz = kind == 2 ? cinfo[5 * c + 1] : 1.0;
            const double t0 = cv ? vv[r0] : 0.0, h0 = cv ? dv[r0] : 0.0;
            double zh = 0.0;
            for (int i = r0 + 1 + l16; i < r1; i += 16) zh = fma(vv[i], dv[i], zh);
            zh = group_reduce<16, false>(zh);
            double zd = 0.0;
            const double i2n = kind == 2 ? 1.0 / (2 * nz) : 0.0, cz = kind == 2 ? t0 * zh / (nz * nz) : 0.0;
            for (int i = r0 + 1 + l16; i < r1; i += 16) {
                if (kind == 1) dv[i] = 0.0;
                else if (kind == 2) { const double w = vv[i]; const double di = (w * h0 + (t0 + nz) * dv[i] - w * cz) * i2n; dv[i] = di; zd = fma(w, di, zd); }
            }
            zd = group_reduce<16, false>(zd);
            if (kind == 2) {
                const double d0 = (nz * h0 + zh) * i2n, zdn = zd / nz, eyd = (d0 + zdn) * M_SQRT1_2, esd = (d0 - zdn) * M_SQRT1_2;
                const double il = 1.0 / (1 - lam), k0c = (esd * (1 - il) - eyd * il) * M_SQRT1_2, kzc = (-esd * (1 - il) - eyd * il) * M_SQRT1_2, inz = 1.0 / nz;
                for (int i = r0 + 1 + l16; i < r1; i += 16) qv2[i] = fma(il, dv[i], vv[i] * inz * kzc);
                if (l16 == 0) { qv2[r0] = fma(il, d0, k0c); dv[r0] = d0; cinfo[5 * c + 2] = eyd; cinfo[5 * c + 3] = esd; }
            } else if (kind == 1 && l16 == 0) dv[r0] = 0.0;
        }
        if constexpr (TRI) {
            // triples, one thread per triple, from the retained W and lambda: h = W^T dy_c, d = lambda h on the rotated rows (a lambda = 1 row: its entry of d_B, taken
            // by eqrow below; a lambda = 0 row: 0), and for a weighted row its weight u = theta h in f = dx + A^T u BY ROW beside the boundary cones' (k_backward_rt:
            // a~ d / (1 - lambda))
            for (int c = tid; c < ntri; c += NTHR) {
                const int r0 = T.eoff + 3 * c;
                const double *Wl = Wt + 9 * c;
                const double h0 = dv[r0], h1 = dv[r0 + 1], h2 = dv[r0 + 2];
#pragma unroll
                for (int a = 0; a < 3; a++) {
                    const double t = Wl[a] * h0 + Wl[3 + a] * h1 + Wl[6 + a] * h2, lam = lamt[3 * c + a];
                    dv[r0 + a] = lam * t;
                    qv2[r0 + a] = rkind[r0 + a] == RK_MIX ? lam / (1 - lam) * t : 0.0;
                }
            }
        }
        if constexpr (PSD && MANY) {
            // PSD blocks, from the retained U and B: h = Q^T dy_c, d = B h on the rotated rows (a B = 1 row: its entry of d_B, taken by eqrow below; a B = 0 row: 0), and
            // for a weighted row its weight u = theta h in f = dx + A^T u BY ROW beside the boundary cones' (k_backward_rt: a~ d / (1 - B))
            __syncthreads();
            psd_rotate_vec(dv, false);
            for (int i = psd0 + tid; i < T.eoff; i += NTHR) {
                const double lam = lamp[i - psd0], t = dv[i];
                dv[i] = lam * t;
                qv2[i] = rkind[i] == RK_MIX ? lam / (1 - lam) * t : 0.0;
            }
        }
        __syncthreads();
        // d_B by equality (the numbering's source array was the elimination's to overwrite: eqrow and ceq are its inverse) -> mu
        for (int i = tid; i < m; i += NTHR) if (rkind[i] == RK_EQ) mu[eqrow[i]] = dv[i];
        for (int c = tid; c < nq; c += NTHR) if (ckind[c] == 2) mu[ceq[c]] = cinfo[5 * c + 2];
        __syncthreads();
        // d~ = B_1^-1 d_B from the in-place inverse (entry (e, i) in row e at the pivot column of i; a dropped row has none): 16 lanes per equality
        for (int e0 = 0; e0 < neq; e0 += NTHR / 16) {
            const int e = e0 + (tid >> 4), part = tid & 15;
            double a = 0.0;
            const int pc = e < neq ? pcol[e] : -1;
            if (pc >= 0) { const double *row = sm + erow[e]; for (int i = part; i < neq; i += 16) { const int pi = pcol[i]; if (pi >= 0) a = fma(row[pi], mu[i], a); } }
            a = group_reduce<16, false>(a);
            if (e < neq && part == 0) dB[e] = pc >= 0 ? a : 0.0;
        }
        __syncthreads();
        // t_q = a_q . x_p = sum_e a_q[p_e] d~_e for the z-rows of the list (the pivot columns of a list row are as loaded): 4 lanes per row
        auto list_t = [&]() {
            for (int q0 = 0; q0 < KW; q0 += NTHR / 4) {
                const int q = q0 + (tid >> 2), part = tid & 3;
                const bool live = q < KW && wsrc[q < KW ? q : 0] >= 0;
                double a = 0.0;
                if (live) { const double *row = sm + wrow[q]; for (int e = part; e < neq; e += 4) { const int pc = pcol[e]; if (pc >= 0) a = fma(row[pc], dB[e], a); } }
                a = group_reduce<4, false>(a);
                if (live && part == 0) tvec[q] = a;
            }
        };
        list_t();
        if constexpr (QP) {          // t_j = p_j . x_p for the rows of P (its pivot columns are untouched) -> ptv, as the many-tangent mode rebuilds it
            for (int j0 = 0; j0 < n; j0 += NTHR / 4) {
                const int j = j0 + (tid >> 2), part = tid & 3;
                double a = 0.0;
                if (j < n) for (int e = part; e < neq; e += 4) { const int pc = pcol[e]; if (pc >= 0) a = fma(Pm[j * n + pc], dB[e], a); }
                a = group_reduce<4, false>(a);
                if (j < n && part == 0) ptv[j] = a;
            }
        }
        __syncthreads();
        // per boundary cone, with a_0 = sqrt 2 a_y - a_z and a_z = sum z-hat_i a_i (neither row is stored any more):  A_c^T u = sqrt 2 u_0 a_y + sum u'_i a_i,
        // u'_i = u_i - u_0 z-hat_i.  The a_y share is a row of B: it moves the multiplier of the cone's equality by sqrt 2 u_0 (behind step 5) and drops out of
        // Z^T f.  The list takes theta q'_i = theta (t_i - z-hat_i (z-hat . t)), so that Z^T H x_p = sum theta q'_i a~_i needs no a_z either.
        for (int c = tid; c < nq; c += NTHR) {
            if (ckind[c] != 2) continue;
            const int r0 = T.qoff[c], r1 = T.qoff[c + 1], qb = cbase[c];
            const double inz = 1.0 / cinfo[5 * c + 1], th = cinfo[5 * c + 4], u0 = qv2[r0];
            double zt = 0.0;
            for (int i = r0 + 1; i < r1; i++) zt = fma(vv[i], tvec[qb + i - r0 - 1], zt);
            zt *= inz;
            for (int i = r0 + 1; i < r1; i++) { const double zhi = vv[i] * inz; qv2[i] -= u0 * zhi; tvec[qb + i - r0 - 1] = th * (tvec[qb + i - r0 - 1] - zhi * zt); }
        }
        if constexpr (TRI) {          // a triple's weighted row is one list row of its own: theta t (eqrow keeps its list entry)
            for (int i = T.eoff + tid; i < m; i += NTHR) if (rkind[i] == RK_MIX) { const int q = eqrow[i]; tvec[q] *= wgt[q]; }
        }
        if constexpr (PSD && MANY) {          // so is a block's weighted row
            for (int i = psd0 + tid; i < T.eoff; i += NTHR) if (rkind[i] == RK_MIX) { const int q = eqrow[i]; tvec[q] *= wgt[q]; }
        }
        __syncthreads();
        // f' = dx + sum u'_i a_i by column: a pivot column keeps f'[piv] (the multipliers want it), a free column takes  dx + sum (u'_i - theta q'_i) a~_i, which
        // lacks only -R^T dx[piv] of the reduced right-hand side Z^T (f' - H x_p).  4 lanes per column, fixed summation order.
        // QP: a free column takes -(P x_p)_j = -t_j as well, and -R^T below meets h[piv] = (dx - P x_p)[piv]: Z^T (f' - (H + P) x_p).
        for (int j0 = 0; j0 < n; j0 += NTHR / 4) {
            const int j = j0 + (tid >> 2), part = tid & 3;
            double a = 0.0, b = 0.0;
            if (j < n) for (int q = part; q < KW; q += 4) {
                const int ws = wsrc[q];
                if (ws >= 0) { const double av = sm[wrow[q] + j]; a = fma(av, qv2[ws], a); b = fma(av, tvec[q], b); }
            }
            a = group_reduce<4, false>(a); b = group_reduce<4, false>(b);
            if (j < n && part == 0) {
                if constexpr (QP) fvec[j] = cmap[j] >= 0 ? (dxi[j] - ptv[j]) + a - b : dxi[j] + a;
                else fvec[j] = dxi[j] + a - (cmap[j] >= 0 ? b : 0.0);
            }
        }
        __syncthreads();
        list_t();          // (tvec holds t again: step 5 adds a~ . x_free to it)
        for (int j = tid; j < n; j += NTHR) {
            if (cmap[j] < 0) continue;
            double a = fvec[j];
            for (int e = 0; e < neq; e++) {
                const int pc = pcol[e];
                if constexpr (QP) { if (pc >= 0) a = fma(-sm[erow[e] + j], dxi[pc] - ptv[pc], a); }
                else if (pc >= 0) a = fma(-sm[erow[e] + j], dxi[pc], a);
            }
            fvec[j] = a;
        }
        __syncthreads();
        // x_free = (Z^T H Z)^-1 rhs out of the accumulator tiles: this lane's entries of its four strip rows against the tile columns, summed over the 16 lanes of a row
        if (wave < NTILE) {
            double rr[NTILE];
#pragma unroll
            for (int J = 0; J < NTILE; J++) { const int colr = 16 * J + lc; rr[J] = colr < nf ? fvec[fcol[colr < nf ? colr : 0]] : 0.0; }
            static_for<4>([&](auto rc) {
                constexpr int r = decltype(rc)::value;
                double sacc = 0.0;
                static_for<NTILE>([&](auto Jc) { constexpr int J = decltype(Jc)::value; sacc = fma(acc[J][r], rr[J], sacc); });
                sacc = group_reduce<16, false>(sacc);
                const int rowi = 16 * wave + lg + 4 * r;
                if (lc == 0 && rowi < nf) rx[fcol[rowi]] = -sacc;
            });
        }
    } else {
    // ---- 5. solution: x_free from the right-hand-side column, x_piv = d~ - R x_free
    if (wave < NTILE) {
        static_for<NTILE>([&](auto Jc) {
            constexpr int J = decltype(Jc)::value;
            static_for<4>([&](auto rc) { constexpr int r = decltype(rc)::value; const int rowi = 16 * wave + lg + 4 * r; if (16 * J + lc == cr && rowi < nf) rx[fcol[rowi]] = acc[J][r]; });
        });
    }
    }
    __syncthreads();
    // q_k = a_k . r_x = t_k + a~_k . x_free for the z-rows of boundary cones (pivot entries of r_x are still 0; the a_z entries of the list are skipped: their
    // storage was the sweep's), x_piv per equality: 4 lanes per row
    for (int q0 = 0; q0 < KW + neq; q0 += NTHR / 4) {
        const int q = q0 + (tid >> 2), part = tid & 3;
        double a0 = 0.0, a1 = 0.0;
        const bool isw = q < KW;
        const bool live = q < KW + neq && (!isw || wsrc[q] >= 0);
        if (live) {
            const double *row = sm + (isw ? wrow[q] : erow[q - KW]);
            for (int j = part; j < n; j += 8) {
                const int j2 = min(j + 4, n - 1);
                const double r0v = row[j], r1v = row[j2], x0 = rx[j], x1 = rx[j2];
                a0 = fma(r0v, x0, a0); a1 = fma(r1v, (j + 4 < n) ? x1 : 0.0, a1);
            }
        }
        const double a = group_reduce<4, false>(a0 + a1);
        if (live && part == 0) {
            if (isw) tvec[q] += a;
            else { const int e = q - KW; dB[e] = (pcol[e] >= 0) ? dB[e] - a : 0.0; }      // x_piv (the entries of the pivot columns -- the in-place inverse -- met r_x = 0)
        }
    }
    __syncthreads();
    // per boundary cone: a_z . r_x = z-hat . (A_z r_x); q of its rows -> qv2 (the union region: the sweep's buffers are dead); the list keeps
    // q'_i = q_i - z-hat_i (a_z . r_x), so that  H r_x = sum over z-rows of theta a_i q'_i  needs no a_z
    for (int c = tid; c < nq; c += NTHR) {
        if (ckind[c] != 2) continue;
        const int r0 = T.qoff[c], r1 = T.qoff[c + 1], qb = cbase[c];
        const double inz = 1.0 / cinfo[5 * c + 1];
        double zq = 0.0;
        for (int i = r0 + 1; i < r1; i++) zq = fma(vv[i], tvec[qb + i - r0 - 1], zq);
        zq *= inz;
        qaz[c] = zq;
        for (int i = r0 + 1; i < r1; i++) { const double qi = tvec[qb + i - r0 - 1]; qv2[i] = qi; tvec[qb + i - r0 - 1] = qi - vv[i] * inz * zq; }
    }
    for (int e = tid; e < neq; e += NTHR) { const int pc = pcol[e]; if (pc >= 0) rx[pc] = dB[e]; }      // r_x[p_e] = x_piv
    __syncthreads();
    // g_e = ((H [+ P]) r_x - f)[p_e] = sum over z-rows of theta a_i[p_e] q'_i - f[p_e]   (16 lanes per equality) -> mu[] (as g)
    for (int e0 = 0; e0 < neq; e0 += NTHR / 16) {
        const int e = e0 + (tid >> 4), part = tid & 15;
        double a = 0.0;
        const int pc = e < neq ? pcol[e] : -1;
        if (pc >= 0) for (int q = part; q < KW; q += 16) { if (wsrc[q] >= 0) a = fma(wgt[q] * sm[wrow[q] + pc], tvec[q], a); }
        if constexpr (QP) { if (pc >= 0) for (int i = part; i < n; i += 16) a = fma(Pm[i * n + pc], rx[i], a); }          // + (P r_x)[p_e]: column p_e of P is as loaded, and P is symmetric
        a = group_reduce<16, false>(a);
        if (e < neq && part == 0) mu[e] = pc >= 0 ? a - fvec[pc] : 0.0;
    }
    __syncthreads();
    // mu = B_1^-T g.  The pivot columns of the eliminated rows hold B_1^-1 (in-place Gauss-Jordan inversion: column p_e carried column e of the accumulated row
    // operations through the later steps): mu_e = sum_i T[i][e] g_i -> dB
    for (int e0 = 0; e0 < neq; e0 += NTHR / 16) {
        const int e = e0 + (tid >> 4), part = tid & 15;
        double a = 0.0;
        const int pc = e < neq ? pcol[e] : -1;
        if (pc >= 0) for (int i = part; i < neq; i += 16) a = fma(sm[erow[i] + pc], mu[i], a);          // (g of a dropped row is 0)
        a = group_reduce<16, false>(a);
        if (e < neq && part == 0) dB[e] = pc >= 0 ? a : 0.0;
    }
    __syncthreads();
    NS_STAMP(8);
    if constexpr (FWD) {
        // ---- FWD epilogue: d_x = r_x, eta_B = -mu; per row eta = W^T d_y, then dy = W lambda eta -> vv, ds = -W (1 - lambda) eta -> dv (dv held g_y):
        //      equality rows dy = eta, ds = 0; eliminated rows (lambda = 0) dy = 0, ds = gamma - a . d_x (their rows of A are untouched: 4 lanes per row);
        //      boundary cones from gamma_y, gamma_s, q_i = a_i . d_x (qv2) and a_z . d_x (qaz), with p = (I - z-hat z-hat^T)(A_z d_x - g_z) = (1 - lambda) eta_perp.
        for (int i0 = 0; i0 < m; i0 += NTHR / 4) {
            const int i = i0 + (tid >> 2), part = tid & 3;
            const bool live = i < m && rkind[i < m ? i : 0] == RK_FREE;
            double a0 = 0.0, a1 = 0.0;
            if (live) {
                const double *row = A + i * lda;
                for (int j = part; j < n; j += 8) {
                    const int j2 = min(j + 4, n - 1);
                    const double r0v = row[j], r1v = row[j2], x0 = rx[j], x1 = rx[j2];
                    a0 = fma(r0v, x0, a0); a1 = fma(r1v, (j + 4 < n) ? x1 : 0.0, a1);
                }
            }
            const double a = group_reduce<4, false>(a0 + a1);
            if (live && part == 0) { dv[i] -= a; vv[i] = 0.0; }
        }
        for (int i = tid; i < m; i += NTHR) if (rkind[i] == RK_EQ) { vv[i] = -dB[eqrow[i]]; dv[i] = 0.0; }
        for (int c = tid; c < nq; c += NTHR) {
            if (ckind[c] != 2) continue;
            const int r0 = T.qoff[c], r1 = T.qoff[c + 1];
            const double inz = 1.0 / cinfo[5 * c + 1], gy = cinfo[5 * c + 2], gs = cinfo[5 * c + 3], th = cinfo[5 * c + 4];
            const double etay = -dB[ceq[c]], zq = qaz[c], zeta = (gy - gs) * M_SQRT1_2;
            const double ayd = pcol[ceq[c]] >= 0 ? gy : 0.0;                      // a_y . d_x = gamma_y (the equality; a dropped row is flagged anyway)
            const double q0 = M_SQRT2 * ayd - zq;                                 // a_0 . d_x
            const double etas = (q0 - zq) * M_SQRT1_2 - gs;                       // a_s . d_x - gamma_s
            for (int i = r0 + 1; i < r1; i++) {
                const double zh = vv[i] * inz, pp = (qv2[i] - zh * zq) - (dv[i] - zh * zeta);
                vv[i] = fma(th, pp, zh * etay * M_SQRT1_2); dv[i] = zh * etas * M_SQRT1_2 - pp;
            }
            vv[r0] = etay * M_SQRT1_2; dv[r0] = -etas * M_SQRT1_2;
        }
        if constexpr (TRI) {
            // a triple's weighted row: eta = (a~ . d_x - gamma) / (1 - lambda) with a~ . d_x from the list (tvec), so dy~ = lambda eta, ds~ = gamma - a~ . d_x; its equality
            // and dropped rows went with the others above.  Behind the barrier one thread per triple rotates back: dy = W dy~, ds = W ds~.
            for (int i = T.eoff + tid; i < m; i += NTHR) {
                if (rkind[i] != RK_MIX) continue;
                const double lam = lamt[i - T.eoff], qd = tvec[eqrow[i]] - dv[i];
                vv[i] = lam * qd / (1 - lam); dv[i] = -qd;
            }
            __syncthreads();
            for (int c = tid; c < ntri; c += NTHR) {
                const int r0 = T.eoff + 3 * c;
                const double *Wl = Wt + 9 * c;
                const double y0 = vv[r0], y1 = vv[r0 + 1], y2 = vv[r0 + 2], s0 = dv[r0], s1 = dv[r0 + 1], s2 = dv[r0 + 2];
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    vv[r0 + i] = Wl[3 * i] * y0 + Wl[3 * i + 1] * y1 + Wl[3 * i + 2] * y2;
                    dv[r0 + i] = Wl[3 * i] * s0 + Wl[3 * i + 1] * s1 + Wl[3 * i + 2] * s2;
                }
            }
        }
        if constexpr (PSD) {
            // a block's weighted row: eta = (a~ . d_x - gamma) / (1 - B) with a~ . d_x from the list (tvec), so dy~ = B eta, ds~ = gamma - a~ . d_x; its equality and
            // dropped rows went with the others above.  Then back per block, both vectors at once on the pairs of waves 0 and 1:  dy_c = Q dy~,  ds_c = Q ds~  with
            // Q r = svec(U smat(r) U^T)  (k_backward_rt's rotation back).
            for (int i = psd0 + tid; i < T.eoff; i += NTHR) {
                if (rkind[i] != RK_MIX) continue;
                const double lam = lamp[i - psd0], qd = tvec[eqrow[i]] - dv[i];
                vv[i] = lam * qd / (1 - lam); dv[i] = -qd;
            }
            __syncthreads();
            for (int c = 0; c < T.ns; c++) {
                const int k = T.sord[c], r0 = T.soff[c], d = k * (k + 1) / 2;
                const double *Um = psdU + c * msq;
                for (int idx = tid; idx < 2 * k * k; idx += NTHR) {
                    const int w = idx / (k * k), e = idx - w * k * k, i = e / k, j = e - i * k, a = i >= j ? i : j, b = i >= j ? j : i;
                    const double v = (w ? dv : vv)[r0 + b * k - (b * (b - 1)) / 2 + (a - b)];
                    psdXW[w * 2 * msq + e] = (a == b) ? v : v * M_SQRT1_2;
                }
                __syncthreads();
                for (int idx = tid; idx < 2 * k * k; idx += NTHR) {          // W = U X
                    const int w = idx / (k * k), e = idx - w * k * k, i = e / k, j = e - i * k;
                    const double *X = psdXW + w * 2 * msq;
                    double acc = 0; for (int a = 0; a < k; a++) acc = fma(Um[i * k + a], X[a * k + j], acc);
                    psdXW[w * 2 * msq + msq + e] = acc;
                }
                __syncthreads();
                for (int idx = tid; idx < 2 * d; idx += NTHR) {              // W U^T, packed back as svec
                    const int w = idx / d, pos = idx - w * d;
                    const double *Wm = psdXW + w * 2 * msq + msq;
                    int b = 0, rem = pos; while (rem >= k - b) { rem -= k - b; b++; }
                    const int a = b + rem;
                    double acc = 0; for (int e = 0; e < k; e++) acc = fma(Wm[a * k + e], Um[b * k + e], acc);
                    (w ? dv : vv)[r0 + pos] = (a == b) ? acc : acc * M_SQRT2;
                }
                __syncthreads();
            }
        }
        __syncthreads();
        if constexpr (REF) {
            // ---- REF epilogue: x+ = x + dx -> rx,  v+ = v + (dy - ds) -> vv,  y+ = Pi(v+) -> tvec,  s+ = y+ - v+.  The elimination overwrote A: the instance's
            //      value row (QP: and its P row) is scattered again for rho at the new point.  The step is kept only when the elimination raised no flag and rho fell below the
            //      rho of the point that came in (as evaluated now AND as recorded when that point was written: the record never increases); else nothing is written.
            const bool flagged = (misc[2] & 4) != 0;
            bool ok = false;
            double rho1 = rho_cur;
            if constexpr (PSD) {
            // PSD: the same test on a SHORTENED step when the full one fails it.  The projection onto a PSD block changes its active set (the signs of the eigenvalues)
            // continuously along the step, and from a loose point the full Newton step can cross such a change and RAISE rho, where the step of a plain cone rarely
            // does (measured: one instance of 48 at eps 1e-4, the dense numpy step raising rho 8.6e-5 -> 2.2e-4 alike).  The step (dx in rx, dv = dy - ds in dv) is kept
            // and tried at alpha = 1, 1/2, 1/4, 1/8: x+ = x + alpha dx -> fvec, v+ = v + alpha dv -> vv, y+ = Pi(v+) -> tvec; the first trial that passes ce_refine's
            // acceptance rule (rho below rho of the point that came in, as evaluated now and as recorded) is written, else nothing is.  alpha = 1 first: where the
            // full step passes, this is ce_refine's step bit for bit in its arithmetic order (fma(1, d, x) = x + d).  A is scattered once for all trials.
            if (!flagged) {          // (uniform)
                const double *vals = Avals + (size_t)inst * T.nnz_aug;
                for (int i = tid; i < m; i += NTHR) dv[i] = vv[i] - dv[i];
                for (int i = tid; i < m * lda; i += NTHR) A[i] = 0.0;
                __syncthreads();
                for (int k0 = tid; k0 < T.nnzA; k0 += 4 * NTHR) {
                    double v0[4]; int r0[4], c0[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) { const int k = k0 + u * NTHR, kc = k < T.nnzA ? k : 0; v0[u] = vals[kc]; r0[u] = T.rowidx[kc]; c0[u] = k < T.nnzA ? T.colidx[kc] : -1; }
#pragma unroll
                    for (int u = 0; u < 4; u++) if (c0[u] >= 0) A[r0[u] * lda + c0[u]] = -v0[u];
                }
                double alpha = 1.0;
                for (int trial = 0; trial < 4 && !ok; trial++, alpha *= 0.5) {          // (uniform: rho1 is the same LDS reduction in every thread)
                    __syncthreads();
                    for (int j = tid; j < n; j += NTHR) fvec[j] = fma(alpha, rx[j], W.x[(size_t)inst * n + j]);
                    for (int i = tid; i < m; i += NTHR) vv[i] = fma(alpha, dv[i], W.y[(size_t)inst * m + i] - W.s[(size_t)inst * m + i]);
                    __syncthreads();
                    project_dual(vv, tvec);
                    __syncthreads();
                    rho1 = kkt_residual(fvec, tvec, vv, false);
                    ok = rho1 < fmin(rho0, rho_cur);
                }
                if (ok) {
                    for (int j = tid; j < n; j += NTHR) W.x[(size_t)inst * n + j] = fvec[j];
                    for (int i = tid; i < m; i += NTHR) { const double yi = tvec[i]; W.y[(size_t)inst * m + i] = yi; W.s[(size_t)inst * m + i] = yi - vv[i]; }
                }
            }
            } else
            if (!flagged) {          // (uniform)
                const double *vals = Avals + (size_t)inst * T.nnz_aug;
                for (int j = tid; j < n; j += NTHR) rx[j] += W.x[(size_t)inst * n + j];
                for (int i = tid; i < m; i += NTHR) vv[i] = (W.y[(size_t)inst * m + i] - W.s[(size_t)inst * m + i]) + (vv[i] - dv[i]);
                for (int i = tid; i < m * lda; i += NTHR) A[i] = 0.0;
                __syncthreads();
                for (int k0 = tid; k0 < T.nnzA; k0 += 4 * NTHR) {
                    double v0[4]; int r0[4], c0[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) { const int k = k0 + u * NTHR, kc = k < T.nnzA ? k : 0; v0[u] = vals[kc]; r0[u] = T.rowidx[kc]; c0[u] = k < T.nnzA ? T.colidx[kc] : -1; }
#pragma unroll
                    for (int u = 0; u < 4; u++) if (c0[u] >= 0) A[r0[u] * lda + c0[u]] = -v0[u];
                }
                load_P();          // (step 2 transformed its rows)
                project_dual(vv, tvec);
                __syncthreads();
                rho1 = kkt_residual(rx, tvec, vv, false);
                ok = rho1 < fmin(rho0, rho_cur);
                if (ok) {
                    for (int j = tid; j < n; j += NTHR) W.x[(size_t)inst * n + j] = rx[j];
                    for (int i = tid; i < m; i += NTHR) { const double yi = tvec[i]; W.y[(size_t)inst * m + i] = yi; W.s[(size_t)inst * m + i] = yi - vv[i]; }
                }
            }
            if (tid == 0) {
                W.rstatus[inst] = rst0 | (ok ? 1 : (flagged ? 4 : 2));
                if (ok) W.steps[inst] += 1;
                if (W.first) W.resid[2 * (size_t)inst] = rho0;
                W.resid[2 * (size_t)inst + 1] = ok ? rho1 : rho_cur;
            }
            return;
        } else {
        if constexpr (MANY) {
            for (int j = tid; j < n; j += NTHR) W.dx[kc * W.sxk + (size_t)inst * n + j] = rx[j];
            for (int i = tid; i < m; i += NTHR) { W.dy[kc * W.syk + (size_t)inst * m + i] = vv[i]; if (W.ds) W.ds[kc * W.syk + (size_t)inst * m + i] = dv[i]; }
            if (tid == 0) {
                const int fl = misc[2];
                if (adjk) adjk[inst] = fl;
                if (W.iters) W.iters[kc * W.sak + inst] = 0;
                if (fix && (fl & 4) && kc == 0) fix[1 + atomicAdd(fix, 1)] = inst;      // listed once for all tangents (the LSQR launch behind ce_jvp_many / ce_jvp_tri_many walks K x list pairs)
            }
            continue;
        } else {
        for (int j = tid; j < n; j += NTHR) W.dx[(size_t)inst * n + j] = rx[j];
        for (int i = tid; i < m; i += NTHR) { W.dy[(size_t)inst * m + i] = vv[i]; if (W.ds) W.ds[(size_t)inst * m + i] = dv[i]; }
        if (tid == 0) {
            const int fl = misc[2];
            if (adj_status) adj_status[inst] = fl;
            if (W.iters) W.iters[inst] = 0;
            if (fix && (fl & 4)) fix[1 + atomicAdd(fix, 1)] = inst;      // rank-deficient system: the LSQR launch behind this kernel re-solves it (ce_jvp)
        }
        return;
        }
        }
    }
    if constexpr (MANY && !FWD) {          // the a_y share of f, taken out of f' above: mu_c = mu'_c - sqrt 2 u_0 (qv2 of a t-row is not step 5's to write)
        for (int c = tid; c < nq; c += NTHR) if (ckind[c] == 2 && pcol[ceq[c]] >= 0) dB[ceq[c]] -= M_SQRT2 * qv2[T.qoff[c]];
        __syncthreads();
    }
    // ---- r_y (as k_backward_rt; the t-row of a boundary cone holds a_y: a_0 . r_x = sqrt 2 (a_y . r_x) - a_z . r_x)
    for (int i = tid; i < z + T.l; i += NTHR) vv[i] = (eqrow[i] >= 0) ? dB[eqrow[i]] : dv[i];
    for (int c = tid; c < nq; c += NTHR) {
        const int r0 = T.qoff[c], r1 = T.qoff[c + 1];
        if (ckind[c] == 0) { for (int i = r0; i < r1; i++) vv[i] = dB[eqrow[i]]; }
        else if (ckind[c] == 1) { for (int i = r0; i < r1; i++) vv[i] = dv[i]; }
        else {
            const double lam = cinfo[5 * c], inz = 1.0 / cinfo[5 * c + 1], eyd = cinfo[5 * c + 2], esd = cinfo[5 * c + 3];
            const double rhoy = dB[ceq[c]];
            const double zq = qaz[c];                                             // z-hat . (A_z r_x) = a_z . r_x
            const double eyq = pcol[ceq[c]] >= 0 ? eyd : 0.0;                     // a_y . r_x = e_y . d (the equality; a dropped row is flagged anyway)
            const double q0 = M_SQRT2 * eyq - zq;                                 // a_0 . r_x
            const double esq = (q0 - zq) * M_SQRT1_2;
            const double il = 1.0 / (1 - lam);
            const double cy = rhoy - il * (eyd - lam * eyq), cs = esd - il * (esd - lam * esq);
            const double k0 = (cy + cs) * M_SQRT1_2, kz = (cy - cs) * M_SQRT1_2;
            for (int i = r0 + 1; i < r1; i++) { const double zh = vv[i] * inz; vv[i] = il * (dv[i] - lam * qv2[i]) + kz * zh; }
            vv[r0] = il * (dv[r0] - lam * q0) + k0;
        }
    }
    if constexpr (TRI) {
        // triples (as k_backward_rt): r~_y on the three rotated rows -- the multiplier of an equality row, d = 0 of a dropped row, (d - lambda a~ . r_x) / (1 - lambda) of a
        // weighted row with a~ . r_x from the list (tvec) -- and back to the original basis, r_y,c = W r~_y,c; one thread per triple
        for (int c = tid; c < ntri; c += NTHR) {
            const int r0 = T.eoff + 3 * c;
            const double *Wl = Wt + 9 * c;
            double rt[3];
#pragma unroll
            for (int a = 0; a < 3; a++) {
                const int i = r0 + a, rk = rkind[i], e = eqrow[i];
                const double lam = lamt[3 * c + a];
                rt[a] = rk == RK_EQ ? dB[e] : (rk == RK_MIX ? (dv[i] - lam * tvec[e]) / (1 - lam) : dv[i]);
            }
#pragma unroll
            for (int a = 0; a < 3; a++) vv[r0 + a] = Wl[3 * a] * rt[0] + Wl[3 * a + 1] * rt[1] + Wl[3 * a + 2] * rt[2];
        }
    }
    if constexpr (PSD && MANY) {
        // PSD blocks (as k_backward_rt): r~_y on the rotated rows -- the multiplier of an equality row, d = 0 of a dropped row, (d - B a~ . r_x) / (1 - B) of a weighted
        // row with a~ . r_x from the list (tvec) -- and back to the original basis per block, r_y,c = Q r~_y,c
        for (int i = psd0 + tid; i < T.eoff; i += NTHR) {
            const int rk = rkind[i], e = eqrow[i];
            const double lam = lamp[i - psd0];
            vv[i] = rk == RK_EQ ? dB[e] : (rk == RK_MIX ? (dv[i] - lam * tvec[e]) / (1 - lam) : dv[i]);
        }
        __syncthreads();
        psd_rotate_vec(vv, true);
    }
    __syncthreads();
    NS_STAMP(9);
    // ---- outputs in the boundary convention: dA_eval = [-dA.data, db[b_idx]], dq_eval = [dc, 0]   (diffcp_if.py:91-92)
    double *const xs = fvec, *const ys = dv;
    // factor mode (the single-cotangent adjoint alone, W.dA_factors: ce_vjp_qp asks for it when k_expand_dA writes the caller's batch-minor dA): every entry of the
    // row is a product of x, y (the forward's outputs), r_x = -dq (written below) and r_y, so r_y[0 .. m) at the head of the instance's row is all the row needs;
    // one contiguous store instead of nnz_aug.  The flag is the launch's: uniform, the barrier below is skipped by all threads or none.
    bool factors = false;
    if constexpr (!FWD && !MANY) factors = W.dA_factors != 0;
    // record mode (the many-cotangent adjoints of every kind, W.rec: ce_vjp_many_params and its QP / TRI / PSD twins): no dA row either; the pair's record (r_y
    // -- in the original basis: vv stands behind the triples' W r~_y and the blocks' rotation above --, r_tau = 0: the elimination pins it, r_x) goes to the record
    // buffer, and k_param_grad behind the launch evaluates the entries the parameter maps touch.  The QP kind writes no dP either (W.dP is null).  Uniform like the flag above.
    bool records = false;
    if constexpr (MANY && !FWD) records = W.rec != nullptr;
    if (factors) {
        double *const dArow = dAk + (size_t)inst * T.nnz_aug;
        for (int i = tid; i < m; i += NTHR) dArow[i] = vv[i];
    } else if (records) {
        if constexpr (MANY && !FWD) {
            double *const rec = W.rec + kc * W.srk + (size_t)inst * W.rpitch;
            for (int i = tid; i < m; i += NTHR) rec[i] = vv[i];
            for (int j = tid; j < n; j += NTHR) rec[m + 1 + j] = rx[j];
            if (tid == 0) rec[m] = 0.0;
        }
    } else {
    for (int j = tid; j < n; j += NTHR) xs[j] = xg[(size_t)inst * n + j];
    for (int i = tid; i < m; i += NTHR) ys[i] = yg[(size_t)inst * m + i];
    __syncthreads();
    {
        constexpr int OU = MANY ? 6 : 8;          // (MANY: the accumulator tiles stay live across the cotangents; eight entries in flight spill beside them)
        double *const dArow = dAk + (size_t)inst * T.nnz_aug;
        const int nnz = T.nnz_aug;
        for (int k0 = tid; k0 < nnz; k0 += OU * NTHR) {
            int ii[OU], jj[OU];
#pragma unroll
            for (int u = 0; u < OU; u++) { const int kk = min(k0 + u * NTHR, nnz - 1); ii[u] = T.rowidx[kk]; jj[u] = T.colidx[kk]; }
            __builtin_amdgcn_sched_barrier(0);
            double xv[OU], rv[OU], vi[OU], yi[OU];
#pragma unroll
            for (int u = 0; u < OU; u++) { const int jc = jj[u] < n ? jj[u] : 0; xv[u] = xs[jc]; rv[u] = rx[jc]; vi[u] = vv[ii[u]]; yi[u] = ys[ii[u]]; }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < OU; u++) {
                const double va = ce_dA_entry(xv[u], vi[u], yi[u], rv[u]);
                const double val = (jj[u] < n) ? va : -vi[u];
                if (k0 + u * NTHR < nnz) dArow[k0 + u * NTHR] = val;
            }
        }
    }
    }
    for (int j = tid; j <= n; j += NTHR) dqk[j * sdqk + inst * sdqb] = (j < n) ? -rx[j] : 0.0;
    if constexpr (QP && MANY && !FWD) {
        // dP = -sym(r_x x^T) through the structure, consecutive lanes on consecutive entries (x and r_x from LDS); a one-triangle entry stands for both matrix
        // entries and takes both shares, as k_backward_rt writes it.  Record mode: k_param_grad evaluates the entries the P map touches from the record (xs is not staged)
        double *const dProw = W.dP + kc * W.sPk + (size_t)inst * W.Q.nnz_p;
        if (!records)
        for (int k = tid; k < W.Q.nnz_p; k += NTHR) {
            const int i = W.prow[k], j = W.pcol[k];
            const double v = ce_dP_entry(rx[i], xs[j], rx[j], xs[i]);
            dProw[k] = (W.p_tri && i != j) ? 2.0 * v : v;
        }
    }
    if (tid == 0) {
        const int fl = misc[2];
        if (adjk) adjk[inst] = fl;
        if (fix && (fl & 4) && kc == 0) fix[1 + atomicAdd(fix, 1)] = inst;      // rank-deficient system: diffcp's LSQR element replaces this answer (ce_vjp_qp); MANY: listed once for all cotangents
    }
    }          // (the cotangents)
#ifdef CE_TIMING
    NS_STAMP(10);
    if (tid < 10) dAo[(size_t)inst * T.nnz_aug + tid] = (double)(tstamp[tid + 1] - tstamp[tid]);
    if (tid == 10) dAo[(size_t)inst * T.nnz_aug + 10] = (double)(n + neq);
    if (tid == 11) dAo[(size_t)inst * T.nnz_aug + 11] = (double)nf;
    if (tid == 12) { dAo[(size_t)inst * T.nnz_aug + 12] = (double)(tsub[0] - tstamp[5]); dAo[(size_t)inst * T.nnz_aug + 13] = (double)(tsub[1] - tsub[0]); dAo[(size_t)inst * T.nnz_aug + 14] = (double)(tsub[2] - tsub[1]); dAo[(size_t)inst * T.nnz_aug + 15] = (double)KW; }
    if (tid >= 16 && tid < 20) dAo[(size_t)inst * T.nnz_aug + tid] = (double)tsub[8 + tid - 16];
#endif
}

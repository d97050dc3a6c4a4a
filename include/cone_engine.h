/*
 * cone_engine.h -- C ABI of the MI355X-native batched cone-program solve + differentiate engine.
 *
 * This is the drop-in boundary underneath the Python solver plugin
 * (cvxpylayers_amd/interfaces/mi355_if.py), which mirrors the reference plugin
 * cvxpylayers/interfaces/diffcp_if.py.  The reference has NO FFI for this path (its arithmetic is
 * in the third-party diffcp/SCS packages, reached through Python calls), so every entry point
 * below cites the reference *call site* whose work it replaces:
 *
 *   ce_create   <- DIFFCP_ctx.__init__            (diffcp_if.py:105-120; interfaces/__init__.py:26-33)
 *                  : keeps the CSC structure of the augmented matrix [A_cvx | b_cvx] and the cone dims.
 *   ce_solve    <- _build_diffcp_matrices + diffcp.solve_and_derivative_batch / solve_only_batch
 *                  (diffcp_if.py:46-70, 365-372): cuts (A,b,c) out of A_eval / q_eval, A = -A_cvx,
 *                  solves every instance, returns primal (B,n), dual (B,m) (+ slack, status).
 *   ce_solve_wave <- the same call site, opt-in for small templates (one instance per wave; see its declaration)
 *   ce_vjp      <- _compute_gradients -> adj_batch(dxs, dys, dss=0)   (diffcp_if.py:73-96, 385-403):
 *                  returns d/dA_eval = [-dA.data, db[b_idx]] and d/dq_eval = [dc, 0].
 *   ce_destroy  <- (garbage collection of DIFFCP_ctx)
 *
 * All data pointers are CALLER-OWNED DEVICE memory (fp64 / int32), valid on the device the handle
 * was created for; `stream` is a hipStream_t (NULL = default stream).  Calls only enqueue work:
 * there is no hidden host synchronisation.  The handle owns workspace only and is not thread-safe
 * (reference contract: one layer, one caller thread -- moreau_if.py:14-15).
 * Return value: 0 on success, negative CE_E_* otherwise; per-instance solver status is written to
 * `status[]` with SCS's codes (1 solved, 2 solved/inaccurate, -1 unbounded, -2 infeasible,
 * -6/-7 inaccurate certificates, -4 failed).
 */
#ifndef CONE_ENGINE_H
#define CONE_ENGINE_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ce_engine *ce_handle;

enum {
    CE_OK = 0,
    CE_E_BADARG = -1,        /* inconsistent template / null pointer */
    CE_E_UNSUPPORTED = -2,   /* template / argument combination not implemented on the selected device path (ce_last_error says which) */
    CE_E_TOO_LARGE = -3,     /* instance does not fit the implemented residency modes */
    CE_E_HIP = -4,           /* a HIP runtime call failed (ce_last_error has the string) */
    CE_E_STATE = -5          /* ce_vjp called without the retained forward state it was asked to reuse */
};

/* One-time, host-side description of the canonical template (what CVXPY's ParamConeProg gives a plugin). */
typedef struct {
    int n;                 /* canonical variables */
    int m;                 /* cone rows */
    int nnz_aug;           /* structural non-zeros of the augmented m x (n+1) matrix [A_cvx | b_cvx] */
    const int *indices;    /* [nnz_aug] CSC row indices   (HOST memory) */
    const int *indptr;     /* [n+2]     CSC column starts (HOST memory); column n holds b */
    int z;                 /* zero-cone rows    (dims_to_solver_dict key "z") */
    int l;                 /* nonnegative rows  ("l") */
    int nq;                /* number of second-order cones */
    const int *q;          /* [nq] SOC dimensions ("q"), layout (t, x) */
    int ns;                /* number of PSD cones ("s") */
    const int *s;          /* [ns] PSD orders; svec lower-tri column-major, sqrt(2) off-diagonals */
    int nep;               /* exponential cones ("ep"): triples (x, y, z), y exp(x/y) <= z, after the PSD blocks (SCS row order z,l,q,s,ep,p) */
    int np;                /* 3-d power cones ("p"): triples (x, y, z), x^a y^(1-a) >= |z|, after the exponential cones */
    const double *p;       /* [np] exponents a in (0, 1); a negative entry -a is the DUAL power cone of exponent a (SCS convention)  (HOST memory) */
    /* optional quadratic objective 1/2 x^T P x (param_prob.reduced_P.problem_data_index, interfaces/__init__.py:27): CSC structure
     * of the n x n matrix P, either one triangle or structurally symmetric; nnz_p = 0: linear objective */
    int nnz_p;
    const int *p_indices;  /* [nnz_p] row indices (HOST memory) */
    const int *p_indptr;   /* [n+1] */
} ce_template;

/* Solver settings; names follow SCS / diffcp keyword arguments (diffcp maps eps -> eps_abs, eps_rel). */
typedef struct {
    double eps_abs, eps_rel, eps_infeas;
    double alpha;          /* over-relaxation, 1.5 */
    double rho_x;          /* 1e-6 */
    double scale;          /* initial dual scale, 0.1 */
    int max_iters;         /* 100000 */
    int normalize;         /* Ruiz + l2 equilibration, 1 */
    int adaptive_scale;    /* 1 */
    int warm_start;       /* != 0: x, y, s hold an initial primal / dual / slack point on entry (SCS warm start: u = (x, y, 1), v = (0, s, 0));
                             instances whose point is not finite start cold.  The reference's DIFFCP plugin exposes this as
                             diffcp's `warm_starts` solve argument; MOREAU as `warm_start` (torch/cvxpylayer.py:464-487) */
    int acceleration_lookback;   /* SCS name; default 10 like SCS (diffcp forwards SCS's defaults, diffcp_if.py:356-367).  0: plain iteration.
                                    > 0: type-I Anderson acceleration of the iteration map with a ONE-pair secant history whatever the
                                    value (profiles/r02/aa_memory.json: iteration counts within 2.5 % of lookback 10 on the BASELINE
                                    configurations) and SCS's residual safeguard.  Honoured where ce_acceleration_available() /
                                    the shared-A kernels implement it; other paths iterate plainly (the Python plugin warns once). */
    int acceleration_interval;   /* applied every this many iterations (SCS default 10) */
} ce_settings;

void ce_default_settings(ce_settings *s);

/* ABI guard.  The structs above carry no size field, so a binding compiled / written against an older header would hand the
 * library short structs.  Bindings must check  ce_abi_version() == CE_ABI_VERSION  and  ce_struct_size(which) == sizeof(their
 * struct)  (which: 0 ce_template, 1 ce_settings) once at load time and refuse to continue otherwise (cvxpylayers_amd/_lib.py
 * does; tests/test_cabi.py checks the stub printed in INTEGRATION.md the same way).  CE_ABI_VERSION is bumped whenever a struct
 * layout, an entry point's signature or the meaning of an argument changes (additions that leave every existing call as it was keep the number: ce_tri_ns_variant and entry 17 of ce_get_plan, then ce_value / ce_value_jvp / ce_value_vjp, then ce_cones_create / ce_cones_destroy / ce_cones_rows / ce_cones_state_len / ce_cone_project / ce_cone_dproject, came under 17, as did ce_lpgd_perturb, ce_lpgd_grad and ce_set_transient_solve, and ce_vjp_many and ce_vjp_many_variant, and ce_jvp_many, ce_jvp_qp_many, ce_jvp_many_variant and ce_jvp_qp_many_variant, and ce_vjp_qp_many and ce_vjp_qp_many_variant, and ce_vjp_tri_many and ce_vjp_tri_many_variant, and ce_jvp_tri_many and ce_jvp_tri_many_variant, and ce_jvp_psd, ce_refine_psd, ce_psd_ns_variant and ce_psd_ns_lds, and ce_vjp_psd_many, ce_jvp_psd_many, ce_vjp_psd_many_variant and ce_jvp_psd_many_variant, and ce_jvp_psd_tri, ce_refine_psd_tri, ce_vjp_psd_tri_many, ce_jvp_psd_tri_many, ce_psd_tri_ns_variant, ce_psd_tri_ns_lds, ce_vjp_psd_tri_many_variant and ce_jvp_psd_tri_many_variant, and ce_vjp_many_params, ce_vjp_params, ce_param_grad_variant and ce_param_grad_records, and ce_vjp_qp_many_params, ce_vjp_tri_many_params, ce_vjp_psd_many_params and ce_vjp_psd_tri_many_params, and ce_solve_wave, ce_wave_variant, ce_wave_lds and ce_wave_occupancy; 16: ce_get_plan appends last_sa_fwd, last_sa_lsqr; 15: ce_refine added; 14: ce_jvp added; 13: ce_jvp_lsqr / ce_jvp_shared_a added; 12: ce_get_plan added; 11: ce_vjp re-solves rank-deficient instances by LSQR when q_vals is given, adj_status is a bit field, ce_set_adjoint_resolve added; 10: ce_vjp_lsqr added; 9: ce_vjp_shared_a takes sA_b and q_vals -- the adjoint system gains diffcp's tau row and column --, its iter_lim default is diffcp's 2 (n + m + 1); 8: ce_set_dispatch_history added, ce_status_summary writes a fourth "ready" int; 7: ce_status_summary added; 6: ce_default_settings = SCS defaults incl. acceleration_lookback 10, ce_acceleration_available). */
#define CE_ABI_VERSION 17
int ce_abi_version(void);
int ce_struct_size(int which);
/* The iterative adjoint solver of ce_vjp_shared_a / ce_vjp_lsqr (the calls that solve EVERY instance iteratively): 0 = LSQR (Paige & Saunders; diffcp's default
 * mode, diffcp_if.py:86), 1 = LSMR (Fong & Saunders; diffcp's mode="lsmr": same operator, same atol / btol / conlim / iter_lim arguments, scipy.sparse.linalg.lsmr's
 * recurrences and stopping tests).  Engine state, default 0; the re-solve of rank-deficient instances inside ce_vjp always runs LSQR.  CE_E_BADARG for other values. */
int ce_set_lsqr_variant(ce_handle h, int variant);
/* 1 when ce_solve / ce_solve_qp on this engine honour ce_settings.acceleration_lookback > 0 (second-generation forward kernel with
 * room for its five extra vectors in LDS; the first-generation and size-generic kernels, which keep them in global memory), else 0: the
 * request is ignored on that engine (plain iteration). */
int ce_acceleration_available(ce_handle h);

int ce_create(const ce_template *tpl, int device, ce_handle *out);
int ce_destroy(ce_handle h);
const char *ce_last_error(void);

/*
 * Forward.  Element (k, i) of the reference's A_eval (nnz_aug x B) is read at A_vals[k*sA_k + i*sA_b];
 * element (k, i) of q_eval ((n+1) x B) at q_vals[k*sq_k + i*sq_b] (strides in elements), so both the
 * reference layout (batch-minor: sA_k = B, sA_b = 1) and the engine-native batch-major layout
 * (sA_k = 1, sA_b = nnz_aug) are accepted; the former costs one transpose pass.
 * Outputs (row-major, contiguous): x [B][n], y [B][m], s [B][m]; iters [B], status [B] int32;
 * resid [B][3] = (primal residual, dual residual, gap) or NULL.
 * The batch-major copy of A_vals and (x,y,s) pointers are retained for ce_vjp(reuse_forward=1).
 */
int ce_solve(ce_handle h, int B,
             const double *A_vals, long sA_k, long sA_b,
             const double *q_vals, long sq_k, long sq_b,
             const ce_settings *settings,
             double *x, double *y, double *s, int *iters, int *status, double *resid,
             void *stream);

/*
 * The same solve, ONE INSTANCE PER WAVE, for small templates (k_fwd_wave; no reference call site: the reference calls SCS per instance whatever the size; additions
 * under ABI 17).  ce_solve gives every instance a workgroup of 256 or 512 threads, whose barriers leave a template of a few tens of rows idle; here a 64-thread
 * workgroup solves an instance, with no workgroup barrier, its vectors in registers and A-hat and the inverse of the reduced matrix in its own LDS.
 *   served      : a linear objective (no P structure), zero / nonnegative / second-order cones of any dimensions, n <= 32, m <= 64, any sparsity pattern.
 *   ce_solve_wave   : arguments, layouts, outputs, status codes, warm start and retention (ce_vjp with A_vals == NULL) of ce_solve; every ce_settings field is honoured
 *                     (acceleration: one secant pair for any positive lookback).  The dispatch history of ce_set_dispatch_history is neither read nor written: the
 *                     kernel takes the instances in index order.  CE_E_UNSUPPORTED on a handle it does not serve, before anything is enqueued and with nothing
 *                     written; ce_last_error names the reason.
 *   ce_wave_variant : the row of the kernel's instantiation list (csrc/ce_variants_wave.h) that serves the handle, -1: not served, or h == NULL.
 *   ce_wave_lds     : the launch's dynamic LDS in bytes (0 when not served).
 *   ce_wave_occupancy: resident workgroups (= instances) per CU of that row at that footprint, as the runtime's occupancy query reports it (0 when not served).
 */
int ce_solve_wave(ce_handle h, int B,
                  const double *A_vals, long sA_k, long sA_b,
                  const double *q_vals, long sq_k, long sq_b,
                  const ce_settings *settings,
                  double *x, double *y, double *s, int *iters, int *status, double *resid,
                  void *stream);
int ce_wave_variant(ce_handle h);
int ce_wave_lds(ce_handle h);
int ce_wave_occupancy(ce_handle h);

/*
 * Backward (vector-Jacobian product), diffcp adjoint with ds = 0 (diffcp_if.py:84).
 * dx [B][n], dy [B][m] contiguous.  Gradients are written in the *boundary* convention
 * dA_vals (k, i) at [k*sdA_k + i*sdA_b] = [-dA.data, db[b_idx]],  dq_vals (k,i) at [k*sdq_k + i*sdq_b] = [dc, 0].
 * If A_vals == NULL the batch-major copy retained by the last ce_solve on this handle is used.
 * The system M^T r = dz is reduced cone block by cone block and eliminated directly with r_tau pinned to 0 (the same gradients as diffcp's LSQR wherever it is
 * regular).  Where it is RANK DEFICIENT (redundant equality rows, degenerate active sets) the elimination only has a basic solution to offer while diffcp's LSQR
 * (diffcp_if.py:86 -> adj_batch) returns the minimum-norm one: with q_vals given (the call's q_eval, as ce_solve; c and b enter diffcp's full (n + m + 1)
 * system through it) such instances -- and instances whose active set exceeds the kernel's tile -- are listed on the device by the elimination kernel and
 * re-solved behind it by the LSQR kernel of ce_vjp_lsqr (one more launch whose workgroups walk the list; no host round trip), so the DEFAULT answer is
 * diffcp's on every instance.  q_vals == NULL, ce_set_adjoint_resolve(h, 0, ...) or a quadratic objective: no re-solve.
 * adj_status [B] (or NULL), bit field: 1 = LSQR re-solve stopped at its iteration limit; 2 = active set larger than the direct solve holds and no re-solve
 * (zero gradient); 4 = rank-deficient system (free variables set to zero by the elimination); 8 = gradients replaced by the LSQR re-solve.
 */
int ce_vjp(ce_handle h, int B,
           const double *A_vals, long sA_k, long sA_b,
           const double *q_vals, long sq_k, long sq_b,
           const double *x, const double *y, const double *s,
           const double *dx, const double *dy,
           double *dA_vals, long sdA_k, long sdA_b,
           double *dq_vals, long sdq_k, long sdq_b,
           int *adj_status,
           void *stream);

/* Layout helper: out (cols x rows, row-major) = transpose of in (rows x cols, row-major), fp64, caller-owned
 * device buffers.  Used by the plugin to turn the reference's batch-minor A_eval (nnz_aug x B) into the
 * engine-native batch-major (B x nnz_aug) once, into a tensor it keeps for backward. */
int ce_transpose(ce_handle h, int rows, int cols, const double *in, double *out, void *stream);

/* Enqueues, behind whatever produced v[] (B int32 on the device: the status of a forward call or the adj_status of a backward call), the reduction
 * summary_host[0] = min_i v[i], [1] = #{i: v[i] == 2}, [2] = #{i: (v[i] & 3) != 0} and its copy to summary_host (FOUR ints of PINNED host memory: the
 * fourth is set to 1 after the three values are visible).  The caller synchronises the stream (or an event) before reading it -- or clears
 * summary_host[3] before the call and polls it.  This is the only host <- device traffic a forward call of the Python plugin needs in order to
 * honour the reference's contract that a failed instance raises SolverError from forward() (diffcp_if.py:365-372 raises inside the call): 12 bytes instead
 * of the status vector.  When summary_host is pinned memory mapped into the device's address space (hipHostMalloc / torch's pin_memory) the kernel stores
 * there directly; any other host pointer goes through one of EIGHT rotating device slots and an asynchronous copy: at most eight such calls may be in flight
 * on the stream between two synchronisations of the caller.
 * LIFETIME: the engine remembers, per 64-byte line of host memory, whether the line is mapped and its device alias (one hipPointerGetAttributes per line,
 * not per call).  A buffer handed to this function must therefore stay allocated AND pinned for as long as the engine lives (or until another line has
 * been passed in between): freeing it and re-using the address for a different allocation leaves the engine with a stale alias. */
int ce_status_summary(ce_handle h, int B, const int *status, int *summary_host, void *stream);

/*
 * Quadratic objective (templates created with nnz_p > 0): ce_solve / ce_vjp with the values of P  <- P_eval of the QP-capable
 * plugins (moreau_if.py:399-404; _quad_form_dpp.py:32).  P_vals is BATCH-MAJOR (B, nnz_p) contiguous device memory (the P entries
 * in the template's structure; for a structurally symmetric P the values must be symmetric).  SCS 3's QP embedding: P joins the
 * reduced KKT matrix, tau-tilde is the positive root of a quadratic, dual residual / gap / objective include P.  ce_vjp_qp also
 * returns dP_vals (B, nnz_p) batch-major (the gradient of a one-triangle entry is that of both matrix entries it stands for).
 * ce_qp_native(h): 1 if this template's quadratic objective runs inside the kernels (fits the register-tiled variants, no
 * PSD / exponential / power cones); otherwise callers reduce it to an epigraph SOC themselves (mi355_if.py QuadEpigraph).
 */
int ce_qp_native(ce_handle h);
int ce_solve_qp(ce_handle h, int B, const double *A_vals, long sA_k, long sA_b, const double *q_vals, long sq_k, long sq_b,
                const double *P_vals, const ce_settings *settings, double *x, double *y, double *s, int *iters, int *status, double *resid, void *stream);
int ce_vjp_qp(ce_handle h, int B, const double *A_vals, long sA_k, long sA_b, const double *P_vals,
              const double *x, const double *y, const double *s, const double *dx, const double *dy,
              double *dA_vals, long sdA_k, long sdA_b, double *dq_vals, long sdq_k, long sdq_b, double *dP_vals, int *adj_status, void *stream);

/*
 * Parameter-map evaluation on the device, batch-major  <- CvxpyLayer.forward's  A_eval = A_map @ p_stack,
 * q_eval = q_map @ p_stack  (torch/cvxpylayer.py:433-451; _ScipySparseMatmul :12-37) and, called with the transposed map,
 * their backward (grad_p_stack = map^T @ grad, :32-37).  The map is CSR (rows x cols; indptr/indices/vals are DEVICE arrays):
 *     out[b*ld_out + r] = sum_{t = indptr[r] .. indptr[r+1]-1} vals[t] * P[b*ld_p + indices[t]]      b < B, r < rows
 * i.e. parameters and results are (B, .) row-major, so the result is already in the engine-native batch-major layout and the
 * reference's p_stack transpose and the layout pass of ce_solve both disappear.  No handle: any device pointer set works.
 */
int ce_parammap_apply(int device, int B, int rows, const int *indptr, const int *indices, const double *vals,
                      const double *P, long ld_p, double *out, long ld_out, void *stream);
/* Same map, with the number of source columns known (cols > 0: when a source row fits LDS it is staged there once per instance,
 * so maps that transpose a matrix parameter stay one pass over HBM) and optional accumulation: accumulate != 0 computes
 * out[b, r] += ... and leaves rows without entries untouched -- the sum of the A-map and q-map gradients into one p_stack
 * gradient (autograd's add in the reference, torch/cvxpylayer.py:32-37 called once per map). */
int ce_parammap_apply2(int device, int B, int rows, int cols, int accumulate, const int *indptr, const int *indices, const double *vals,
                       const double *P, long ld_p, double *out, long ld_out, void *stream);

/*
 * Constant-A path (A batch-invariant; only b, c vary): the matrix products of the iteration are batch GEMMs done by the
 * caller with rocBLAS (cvxpylayers_amd/interfaces/const_a.py); these entry points are the per-instance elementwise part.
 * All vectors are (B, lp) row-major with layout (x[n] | y[m] | tau); per-instance scalars are arrays of length B.
 *   ce_ca_step   : tau-tilde, u-tilde, cone projection, (optionally) relaxed update + renormalisation of w
 *   ce_ca_check  : termination test / certificates / adaptive scale of a check iteration, then that iteration's update
 *   ce_ca_psd    : in-place projection of the PSD blocks of U (the step kernel leaves the cone input there)
 *   ce_ca_finish : classification of unfinished instances and un-normalised write-back of x (B,n), y (B,m), s (B,m)
 * They replace the same steps of diffcp.solve_and_derivative_batch -> SCS (diffcp_if.py:365-372) as ce_solve does.
 */
int ce_ca_step(ce_handle h, int B, int lp, double *W, double *UT, double *U, const double *PX, long ld_px, const double *QY, long ld_qy,
               const double *G, const double *PHI, const double *scale, const double *inv_den, const int *active,
               int update_w, int norm_after, double alpha, void *stream);
int ce_ca_check(ce_handle h, int B, int lp, int iter, const ce_settings *settings, double *W, const double *UT, const double *U,
                const double *AX, long ld_ax, const double *ATY, long ld_aty, const double *D, const double *E,
                const double *b_hat, const double *c_hat, const double *sigma, const double *nrm_b0, const double *nrm_c0,
                double *scale, double *sum_log, int *n_log, int *last_scale_iter, int *active, int *status, int *iters,
                double *resid, int *rescaled, void *stream);
int ce_ca_psd(ce_handle h, int B, int lp, double *U, const int *active, void *stream);
/* The same projection on the matrix cores (v_mfma_f64_16x16x4_f64), warm-started from the eigenvectors of the previous call: Vstate
 * (B, ns, maxs * maxs; row-major k x k per block) is caller-owned state, warm = 0: no previous call.  Warm calls REFINE the previous
 * decomposition (R = I - V^T V, D = V^T S V, first-order correction V <- V + V E, quadratically convergent, orthogonality self-correcting:
 * no periodic restart needed) and fall back to Jacobi sweeps when a correction would leave the basin of the first-order step.  warm: 0 cold, 1 warm;
 * bit 1 (warm = 3) is a debugging switch: warm-started Jacobi sweeps only, no refinement (scripts/psd_refine_debug.py).  PSD orders <= 39. */
int ce_ca_psd_mfma(ce_handle h, int B, int lp, double *U, double *Vstate, int warm, const int *active, void *stream);
/* Exponential / power cone triples of the cone input U (B, lp) projected in place (after ce_ca_step, like ce_ca_psd); roots
 * (B, nep + np) is caller-owned state: each cone's root of the previous iteration (zero-initialised). */
int ce_ca_triples(ce_handle h, int B, int lp, double *U, double *roots, const int *active, void *stream);
/* J (B, nep + np, 9): the 3x3 Jacobians of that projection at v = y - s (rows of v have pitch ld_v), used by the batched-LSQR
 * adjoint of the constant-A path in place of diffcp's per-instance dpi operator (diffcp_if.py:86 -> adj_batch). */
int ce_ca_triple_jac(ce_handle h, int B, const double *v, long ld_v, double *J, void *stream);
/* w += alpha (u - ut) (+ renormalisation) as its own launch, for templates whose PSD blocks are projected after ce_ca_step */
int ce_ca_update(ce_handle h, int B, int lp, double *W, const double *UT, const double *U, const int *active, int norm_after, double alpha, void *stream);
int ce_ca_finish(ce_handle h, int B, int lp, int max_iters, const double *W, const double *UT, const double *U, const double *D,
                 const double *E, const double *b_hat, const double *c_hat, const double *sigma, const double *scale,
                 const int *active, int *status, int *iters, double *x, double *y, double *s, void *stream);

/*
 * Shared-A forward  <- _build_diffcp_matrices + diffcp.solve_and_derivative_batch (diffcp_if.py:46-70, 365-372) for templates whose A does
 * not depend on the parameters and consists of r <= 64 rows with several entries plus rows with a single entry: the whole solve of an
 * instance in one persistent kernel (iterates in LDS, reduced KKT matrix = diagonal + rank r applied by the Woodbury identity, its
 * r x r core formed on the matrix cores, termination / adaptive scale in the kernel, PSD projection with MFMA contractions).
 * The caller equilibrates the ONE shared matrix (cvxpylayers_amd/interfaces/const_a.py) and passes, all device memory:
 *   AdT (n, RP) row-major: the equilibrated dense rows transposed (solver sign A = -A_cvx), zero padded to RP in {16, 32, 64};
 *   drow (r): their row indices; srow_col / srow_val (m): column (-2 - a: the dense row in slot a, -1: empty row) and value of every single-entry row;
 *   scol_ptr (n + 1) / scol_row: the single-entry rows of every column; gs (n): sum over them of d0_i a_i^2 (d0 = 1000 on zero-cone rows);
 *   Dv (m), Ev (n): the equilibration; b_hat (B, m), c_hat (B, n), sigma / nrm_b0 / nrm_c0 (B): normalised data as in ce_ca_check;
 *   warm_x / warm_y / warm_s: (B, .) initial point used when settings->warm_start != 0, else NULL.
 * Outputs as ce_solve.  CE_E_UNSUPPORTED / CE_E_TOO_LARGE: callers use the batch-GEMM path of const_a.py instead.
 */
int ce_solve_shared_a(ce_handle h, int B, int r, int RP, const double *AdT, const int *drow, const int *srow_col, const double *srow_val,
                      const int *scol_ptr, const int *scol_row, const double *gs, const double *Dv, const double *Ev, const double *b_hat,
                      const double *c_hat, const double *sigma, const double *nrm_b0, const double *nrm_c0, const ce_settings *settings,
                      const double *warm_x, const double *warm_y, const double *warm_s,
                      double *x, double *y, double *s, int *iters, int *status, double *resid, void *stream);

/*
 * Shared-A adjoint  <- _compute_gradients -> adj_batch (diffcp_if.py:73-96, 385-403) for templates whose A does not depend on the
 * parameters: diffcp's adjoint system (r_tau = 0) solved by LSQR -- diffcp's own default mode -- entirely inside one kernel, one
 * workgroup per instance, A applied from its sparse structure, the PSD cone's derivative on the matrix cores.  A_vals0: the nnz_aug
 * boundary values of instance 0 (the A part is shared); instance i's b entries are read at A_vals0 + i * sA_b (sA_b = nnz_aug for a batch-major
 * value matrix, 0 when b is shared too); q_vals: c of instance i at [j * sq_k + i * sq_b] (as ce_solve).  With q_vals the system is diffcp's
 * FULL (n + m + 1) adjoint system, tau row and column included -- on rank-deficient systems LSQR's minimum-norm solution is then diffcp's;
 * q_vals == NULL pins r_tau = 0 (the n + m system of ABI <= 8: the same gradients wherever the system is regular).
 * x, y, s, dx, dy as ce_vjp; dA_bm (B, nnz_aug) batch-major; dq at
 * [k * sdq_k + i * sdq_b]; adj_status[i] = 1 when LSQR hit iter_lim (0: diffcp's 2 (n + m + 1)); lsqr_iters (B) or NULL; atol / btol: LSQR stopping
 * tolerances (diffcp runs 1e-8 / 1e-8: the plugin's default, solver_args lsqr_atol / lsqr_btol / lsqr_iter_lim override); conlim: LSQR stops when its estimate
 * of cond(M^T) exceeds it (diffcp / scipy default 1e8; <= 0 disables the test).  The engine refills its own scratch (split of this call's A values) on `stream`: one engine, one stream at a time.  All cone types (zero / nonnegative / second-order / PSD / exponential / power: the triples' derivative is a symmetrised
 * 3 x 3 block computed once per call); CE_E_TOO_LARGE when the LSQR vectors of one instance exceed LDS (callers fall back to the batched
 * path of const_a.py).
 */
int ce_vjp_shared_a(ce_handle h, int B, const double *A_vals0, long sA_b, const double *q_vals, long sq_k, long sq_b,
                    const double *x, const double *y, const double *s, const double *dx, const double *dy,
                    double *dA_bm, double *dq_vals, long sdq_k, long sdq_b, int *adj_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream);

/*
 * diffcp's LSQR adjoint for templates whose A DOES depend on the parameters  <- adj_batch(..., mode="lsqr"), the mode diffcp_if.py:86 runs by default.
 * ce_vjp solves the adjoint system by a rank-revealing direct elimination (the same gradients wherever the system is regular: every BASELINE configuration);
 * on a rank-deficient system it returns a basic solution where diffcp's LSQR returns the minimum-norm one.  This entry runs ce_vjp_shared_a's LSQR kernel with
 * the A part read per instance: A_vals_bm (B, nnz_aug) batch-major (sA_b = nnz_aug), every other argument as ce_vjp_shared_a.  The plugin selects it with
 * solver_args mode="lsqr".  A is streamed from L2 / HBM twice per LSQR iteration: the direct elimination stays the default for speed.
 */
int ce_vjp_lsqr(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                const double *x, const double *y, const double *s, const double *dx, const double *dy,
                double *dA_bm, double *dq_vals, long sdq_k, long sdq_b, int *adj_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream);

/*
 * FORWARD derivative of the solution map (diffcp's `derivative` / D of solve_and_derivative).  The reference plugin never calls it: diffcp_if.py differentiates in
 * reverse mode only (adj_batch, diffcp_if.py:86), so there is no reference call site; the system and its conventions are diffcp's own (cone_program.py `derivative`:
 * M d = -dQ pi by LSQR, then dx = d_x - x d_tau, dy = DPi d_y - y d_tau, ds = DPi d_y - d_y - s d_tau) and the adjoint entries above are its transpose.
 * One workgroup per instance runs ce_vjp_lsqr's kernel with the two operator applications of the Golub-Kahan process swapped (LSQR recurrences only: ce_set_lsqr_variant
 * does not apply).  A_vals_bm / sA_b, q_vals, x, y, s, atol / btol / conlim / iter_lim as ce_vjp_lsqr; q_vals == NULL pins d_tau = 0 and drops the tau row.
 * Tangents in the boundary convention: tA_vals_bm (B, nnz_aug) batch-major rows stA_b apart (tangent of A_eval = [-A.data, b]), tq_vals at [k * stq_k + i * stq_b]
 * (tangent of q_eval = [c, 0]; the last entry is ignored); a NULL tangent is zero.  Outputs dx (B, n), dy (B, m), ds (B, m; may be NULL) batch-major;
 * jvp_status[i] = 1 when LSQR hit iter_lim; lsqr_iters (B) or NULL.  Enqueues on `stream` only, never synchronises the host.
 * CE_E_TOO_LARGE when the LSQR vectors of one instance exceed LDS; CE_E_UNSUPPORTED for a template whose quadratic objective runs inside the kernels
 * (ce_qp_native: differentiate the epigraph cone form instead).
 * ce_jvp_shared_a: the template's A part is shared (A_vals0 / sA_b as ce_vjp_shared_a, the split products): only the b entries of the tangent rows are read.
 */
int ce_jvp_lsqr(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                const double *x, const double *y, const double *s,
                const double *tA_vals_bm, long stA_b, const double *tq_vals, long stq_k, long stq_b,
                double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream);
int ce_jvp_shared_a(ce_handle h, int B, const double *A_vals0, long sA_b, const double *q_vals, long sq_k, long sq_b,
                    const double *x, const double *y, const double *s,
                    const double *tA_vals_bm, long stA_b, const double *tq_vals, long stq_k, long stq_b,
                    double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream);
/*
 * The forward derivative by DIRECT ELIMINATION, what ce_vjp is to ce_vjp_lsqr: with d_tau pinned to 0 the system M d = -dQ pi reduces, cone block by cone block, to the
 * saddle system of ce_vjp's search-free null-space elimination (the transposed block: same reduced Hessian and equality rows, another right-hand side and
 * epilogue), solved by the same kernel; behind it a fixed grid of ce_jvp_lsqr's workgroups re-solves, on the device, the instances the elimination found rank
 * deficient with diffcp's LSQR under atol / btol / conlim / iter_lim (no host round trip).  Arguments, conventions and outputs as ce_jvp_lsqr (per-instance A).
 * jvp_status[i] is ce_vjp's bit field: 0 solved directly (lsqr_iters[i] = 0); 4 | 8 = rank deficient, re-solved by LSQR (bit 0: it hit iter_lim; lsqr_iters[i] > 0).
 * Templates with exponential and / or 3-d power triples (primal and dual entries) beside zero / nonnegative / second-order cones are served by the same kernel with
 * the triples' code (ce_tri_ns_variant(h) >= 0): a triple's D Pi is diagonalised, its three rows are rotated into that basis and join the equalities, drop out or
 * enter the reduced Hessian as one weighted row; the re-solve list behind it is the same.  On such a template 4 | 8 has a second meaning: a REGULAR instance with a
 * weighted triple row whose eigenvalue lies within 1e-5 of 1 (csrc/ce_backward_ns.h NS_TRI_STIFF) is listed too, because the elimination loses accuracy there (its
 * sweep has no pivot search; error about 0.03 eps / (1 - lambda)^2), and comes back with LSQR's answer, 4 | 8 and lsqr_iters[i] > 0.  The threshold rests on that one
 * law, measured on one shape (problems.CONFIGS["E"], 48 instances); ce_refine does not apply it (the safeguard judges its steps).
 * CE_E_UNSUPPORTED when the template has no search-free elimination (ce_adjoint_ns_variant(h) < 0 and ce_tri_ns_variant(h) < 0: PSD cones, n > 108, a quadratic
 * objective inside the kernels) or the LSQR vectors of one instance exceed LDS: callers use ce_jvp_lsqr.
 */
int ce_jvp(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
           const double *x, const double *y, const double *s,
           const double *tA_vals_bm, long stA_b, const double *tq_vals, long stq_k, long stq_b,
           double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream);

/*
 * NEWTON REFINEMENT of solutions by ce_jvp's elimination.  For a point (x, y, s) let v = y - s, y^ = Pi(v) (the projection onto the dual cone), s^ = y^ - v: a
 * complementary pair in the cones by construction.  The KKT residual there is  F_x = A^T y^ + c,  F_y = A x + s^ - b  (A = -A_vals, b = A_vals[b entries],
 * c = q_vals[:n]),  rho = max(|F_x|_inf, |F_y|_inf) / (1 + max(|b|_inf, |c|_inf)).  One step solves the Jacobian system of (x, v) -> F,
 *        A^T D dv = -F_x,    -A dx + (I - D) dv = F_y        (D = DPi(v)),
 * which is ce_jvp's system with the residual in the place of dQ pi, by the same search-free elimination (one launch of the same kernel with another prologue and
 * epilogue), and moves to  x+ = x + dx,  v+ = v + dv,  y+ = Pi(v+),  s+ = y+ - v+.
 * SAFEGUARD: the step is kept only if rho(x+, y+, s+) < rho(x, y^, s^); otherwise the instance keeps its point bit for bit and takes no further step.  The same
 * holds for an instance the elimination flags (a redundant equality row, a vanishing pivot of the reduced Hessian, more active rows than variables: no LSQR
 * re-solve runs here) and for instances whose forward status is negative (status may be NULL: every instance is refined).  The returned point never has a
 * larger rho than the one that came in.
 * x (B, n), y, s (B, m) batch-major, updated IN PLACE; A_vals_bm (B, nnz_aug) contiguous batch-major rows (sA_b = nnz_aug); q_vals as ce_solve.
 * refine_status[i] bits: 1 at least one step kept, 2 a step rejected by the safeguard, 4 flagged by the elimination, 16 skipped (failed forward status).
 * steps_taken[i]: steps kept.  resid (B, 2): rho before the first step, rho of the returned point (NaN, NaN for a skipped instance).
 * Enqueues `steps` launches on `stream` (steps = 0: none, the outputs are not written) and never synchronises the host.
 * With ce_set_profiling on, the launches are bracketed under class 1 (the adjoint's kernel family: it is that kernel), although the plugin calls this inside forward().
 * Exponential / power triples as ce_jvp (ce_tri_ns_variant(h) >= 0): y^ of a triple is the engine's own projection onto the triple's dual cone, and D comes from
 * the same evaluation.
 * CE_E_UNSUPPORTED as ce_jvp: no search-free elimination (ce_adjoint_ns_variant(h) < 0 and ce_tri_ns_variant(h) < 0: PSD cones, n > 108) or a quadratic objective
 * inside the kernels.  CE_E_BADARG for rows that are not contiguous batch-major.
 */
int ce_refine(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
              double *x, double *y, double *s /* in/out */, const int *status /* may be NULL */, int steps,
              int *refine_status, int *steps_taken, double *resid, void *stream);

/*
 * ce_jvp and ce_refine for a template whose QUADRATIC OBJECTIVE runs inside the kernels (ce_qp_native(h) == 1): the same search-free elimination with P in the
 * stationarity row,  P d_x + A^T D d_v = -g_x,  g_x = tP x + tA^T y + tc  (refinement: F_x = P x + A^T y^ + c), i.e. the reduced Hessian Z^T (H + P) Z.
 * P_vals, tP_vals (B, nnz_p) batch-major in the structure order of ce_create (a one-triangle structure: one entry stands for both matrix entries, in the values
 * and in the tangent); tP_vals, tA_vals_bm, tq_vals may each be NULL (zero).  Other arguments as ce_jvp / ce_refine; ce_jvp_qp takes no q_vals and no LSQR
 * rule: no LSQR has a P term, so NO re-solve runs behind it.  One launch (ce_refine_qp: `steps` launches), never a host synchronisation.
 * jvp_status[i]: 0 solved; 4 the elimination flagged the instance (a redundant equality row, a vanishing pivot of Z^T (H + P) Z, more active rows than
 * variables) and its dropped-variable answer stands, finite -- the contract of ce_vjp_qp; bit 8 is never set and lsqr_iters[i] = 0.  With no active row the
 * reduced Hessian is P alone: regular for a positive definite P.  ce_refine_qp: a flagged instance keeps its point, as in ce_refine.
 * CE_E_UNSUPPORTED when ce_qp_native(h) == 0 or ce_qp_ns_variant(h) < 0.  ce_jvp, ce_jvp_lsqr and ce_refine keep refusing such a handle.
 */
int ce_jvp_qp(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *P_vals,
              const double *x, const double *y, const double *s,
              const double *tA_vals_bm, long stA_b, const double *tq_vals, long stq_k, long stq_b, const double *tP_vals,
              double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters, void *stream);
int ce_refine_qp(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b, const double *P_vals,
                 double *x, double *y, double *s /* in/out */, const int *status /* may be NULL */, int steps,
                 int *refine_status, int *steps_taken, double *resid, void *stream);
/* >= 0: the row of csrc/ce_variants.h CE_NS_VARIANTS that serves ce_jvp_qp / ce_refine_qp (planned on bwd_ns_qp_lds_bytes_of: the dense P on top of
 * ce_adjoint_ns_variant's footprint, two workgroups per CU at the config-2 shape); -1: none (not qp_native, n > 108, CE_BWD_NS=0).  ce_adjoint_ns_variant stays
 * -1 for a qp_native template: its adjoint keeps the pivoting kernel. */
int ce_qp_ns_variant(ce_handle h);
/* >= 0: the row of CE_NS_VARIANTS that serves ce_jvp / ce_refine for a template with exponential / power triples (zero / nonnegative / second-order cones beside
 * them, no PSD block, linear objective, n <= 108; planned on the footprint with the triples' eigenvectors and eigenvalues on top, and only when the LSQR vectors
 * of ce_jvp's re-solve fit LDS); -1: none.  ce_adjoint_ns_variant stays -1 for such a template: its adjoint keeps the pivoting kernel. */
int ce_tri_ns_variant(ce_handle h);

/*
 * ce_jvp and ce_refine for a template with PSD BLOCKS beside zero / nonnegative / second-order cones (linear objective, no exponential / power triple, n <= 108):
 * the same search-free elimination with the blocks' code, behind entry points of their own -- ce_jvp and ce_refine keep refusing such a handle, so nothing changes
 * for a caller that does not ask.  Per block smat(v_c) = U Lambda U^T (the workgroup's Jacobi sweeps); in the basis E_ab = svec(sym(u_a u_b^T)) D Pi(v_c) is diagonal
 * with eigenvalue B_ab = 1 (both eigenvalues positive), 0 (both non-positive) or l+ / (l+ - l-), the comparisons of ce_vjp's pivoting kernel without a snap.  The
 * block's rows of A are rotated into that basis and join the equalities (B = 1), drop out (B = 0) or enter the reduced Hessian as one weighted row each
 * (theta = B / (1 - B)); the answers are rotated back.  ce_refine_psd: y^ of a block is svec(U max(Lambda, 0) U^T) from the same decomposition.
 * ce_refine_psd keeps ce_refine's acceptance rule and adds a shortened step: when the full Newton step fails the rule (a block's active set can change inside the
 * step) the same step is tried at 1/2, 1/4 and 1/8 of its length and the first trial that passes is kept; bit 2 is set only when all four fail.
 * Arguments, outputs, status bits, the re-solve list behind ce_jvp_psd and the safeguard of ce_refine_psd otherwise as ce_jvp / ce_refine.  4 | 8 of ce_jvp_psd has the second
 * meaning it has with triples: an instance with a weighted PSD row of 1 - B < 1e-5 (a small negative eigenvalue beside a large positive one) is handed to LSQR.
 * That threshold is the triples' (csrc/ce_backward_ns.h NS_TRI_STIFF), carried over: the law behind it belongs to the sweep, but it was NOT measured on PSD rows.
 * ce_refine_psd does not apply it.
 * CE_E_UNSUPPORTED when ce_psd_ns_variant(h) < 0.
 */
int ce_jvp_psd(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
               const double *x, const double *y, const double *s,
               const double *tA_vals_bm, long stA_b, const double *tq_vals, long stq_k, long stq_b,
               double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream);
int ce_refine_psd(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                  double *x, double *y, double *s /* in/out */, const int *status /* may be NULL */, int steps,
                  int *refine_status, int *steps_taken, double *resid, void *stream);
/* >= 0: the row of CE_NS_VARIANTS that serves ce_jvp_psd / ce_refine_psd (at least one PSD block, no triple, linear objective, n <= 108; planned on the footprint
 * with the blocks' U, Lambda, B and scratch on top, and only when the LSQR vectors of the re-solve fit LDS); -1: none, or h == NULL.  ce_psd_ns_lds: that
 * footprint in bytes, 0 when there is none.  ce_adjoint_ns_variant and ce_tri_ns_variant stay -1 for such a template, and ce_get_plan does not report these two. */
int ce_psd_ns_variant(ce_handle h);
long ce_psd_ns_lds(ce_handle h);

/*
 * THE OPTIMAL VALUE and its derivatives by the envelope theorem.  No reference call site: the reference's layers return the minimiser and the duals, and users
 * rebuild the value from x in torch and back-propagate through the adjoint (diffcp_if.py:385-403).  At a solution (x, y) of
 *        min c^T x + d + 1/2 x^T P x   s.t.  A x + s = b, s in K                (A = -A_vals, b = A_vals[b entries], c = q_vals[:n], d = q_vals[n])
 * the value p* = c^T x + d + 1/2 x^T P x has the PARTIAL derivatives of the Lagrangian as its total derivatives:  dp/dA = y x^T, dp/db = -y, dp/dc = x,
 * dp/dd = 1, dp/dP = 1/2 x x^T.  No linear system is solved (nothing can be rank deficient), every cone kind and every path of the engine is served, and the
 * cost is one streaming pass.  In the boundary convention A_eval = [-A.data, b]:  dp/dA_eval[k] = -y_row x_col for an A entry, -y_row for a b entry.
 * The A structure comes from the handle; the P STRUCTURE IS PASSED EXPLICITLY: p_rows, p_cols [nnz_p] DEVICE int arrays, row and column of every entry (NULL / 0:
 * linear objective), so that the same entry points serve a handle with P inside the kernels and the epigraph form, whose engine is built on the augmented
 * template and does not know the original P.  A structure with every entry on or above (or on or below) the diagonal is read as one triangle: an off-diagonal
 * entry counts twice, in the value and in dP (ce_vjp_qp's convention); entries out of range count as zero.  P_vals, tP_vals, dP_vals: (B, nnz_p) batch-major.
 * x [B][n], y [B][m] contiguous; the calls enqueue only, never synchronise the host and need no retained forward state.  With ce_set_profiling on the launches are
 * bracketed under class 2 (streaming passes), never class 1: they are not the adjoint's kernels.
 *   ce_value     : pobj[i] = c^T x + d + 1/2 x^T P x,  dobj[i] = -b^T y - 1/2 x^T P x + d  (equal at a solution; A_vals / q_vals with strides as ce_solve, only the
 *                  b entries of A_vals are read).  The sums run in a fixed order: an instance's result depends neither on B nor on its position in the batch.
 *   ce_value_jvp : tval[i] = tc^T x + td + 1/2 x^T tP x - sum_k tA_eval[k] (y_row x_col | y_row): the tangent of p* for tangents in the boundary convention,
 *                  tA_vals_bm (B, nnz_aug) batch-major rows stA_b apart, tq_vals at [k * stq_k + i * stq_b] (ALL n + 1 entries count: d is the last), tP_vals;
 *                  a NULL tangent is zero.  Same fixed order.
 *   ce_value_vjp : for an upstream cotangent g [B]:  dA_vals (k, i) at [k*sdA_k + i*sdA_b] = -g_i y[i, row_k] x[i, col_k] (A entry) / -g_i y[i, row_k] (b entry);
 *                  dq_vals (j, i) at [j*sdq_k + i*sdq_b] = g_i x[i, j], (n, i) = g_i;  dP_vals[i, k] = g_i (1/2 | 1) x_row x_col.  Each output may be NULL (not
 *                  wanted).  dA: batch-major (sdA_k = 1, sdA_b >= nnz_aug; one workgroup per four instances, lanes over the entries) or batch-minor (sdA_b = 1,
 *                  sdA_k >= B; tiles of 64 instances, lanes over the instances): both store whole 512-byte runs and neither needs a ce_transpose behind it.
 *                  skip [B] bytes or NULL: an instance with skip[i] != 0 gets exact zeros in every output, whatever its x, y, g hold (NaN included).
 * CE_E_TOO_LARGE when x and y of one (ce_value) / four (ce_value_vjp) instances exceed LDS.
 */
int ce_value(ce_handle h, int B, const double *A_vals, long sA_k, long sA_b, const double *q_vals, long sq_k, long sq_b,
             const double *P_vals, const int *p_rows, const int *p_cols, int nnz_p, const double *x, const double *y, double *pobj, double *dobj, void *stream);
int ce_value_jvp(ce_handle h, int B, const double *tA_vals_bm, long stA_b, const double *tq_vals, long stq_k, long stq_b,
                 const double *tP_vals, const int *p_rows, const int *p_cols, int nnz_p, const double *x, const double *y, double *tval, void *stream);
int ce_value_vjp(ce_handle h, int B, const double *x, const double *y, const double *g, const unsigned char *skip,
                 double *dA_vals, long sdA_k, long sdA_b, double *dq_vals, long sdq_k, long sdq_b,
                 double *dP_vals, const int *p_rows, const int *p_cols, int nnz_p, void *stream);

/*
 * THE TERMINATION TEST AT A GIVEN POINT.  The forward kernels stop an instance when (ce_forward_v2.h, oracle/cone_oracle.c; tau = 1 here)
 *        res_pri  = |A x + s - b|_inf      <=  eps_abs + eps_rel max(|A x|_inf, |s|_inf, |b|_inf)
 *        res_dual = |P x + A^T y + c|_inf  <=  eps_abs + eps_rel max(|A^T y|_inf, |c|_inf, |P x|_inf)
 *        gap      = |x^T P x + c^T x + b^T y|  <=  eps_abs + eps_rel max(|c^T x|, |b^T y|, |x^T P x|)
 * (A = -A_vals, b = A_vals[b entries], 0 on a row without one, c = q_vals[:n]).  ce_check_solved evaluates exactly that at a point the CALLER supplies, so that a
 * point obtained without the solver -- a warm start moved by ce_refine (solver_args newton_first) -- can be accepted under the solver's own
 * rule.  The cone conditions are NOT tested: the affine test is sufficient only for a complementary pair in the cones, which is what ce_refine returns for an
 * instance that kept a step (refine_status & 1).  Pass that vector as `eligible` with eligible_mask = 1: an instance with (eligible[i] & eligible_mask) == 0 is
 * unsolved whatever its residual (eligible = NULL: every instance is tested).
 * A_vals, q_vals with strides as ce_solve (any pair; nothing is copied); the P structure explicit, as ce_value (one triangle: an off-diagonal entry counts twice;
 * NULL / 0: linear objective); P_vals (B, nnz_p) batch-major; x [B][n], y, s [B][m] contiguous.
 *   solved instance : solved[i] = 1, status[i] = 1, iters[i] = 0, resid[3 i ..] = res_pri, res_dual, gap
 *   any other       : solved[i] = 0; status[i], iters[i] and its resid row are NOT touched
 *   n_unsolved[0]   : set (not accumulated) to the number of unsolved instances -- a DEVICE int; the caller copies it where it needs it
 * A non-finite entry in the point, the values or the products makes its own instance unsolved and nothing else.  One workgroup per instance; every sum runs in an
 * order fixed by the template and the thread count (no floating-point atomics), so an instance's numbers depend neither on B nor on its position in the batch.
 * The instance's value row is read from memory once and staged in LDS when the workgroup's footprint stays within 64 KB; a longer row is read twice (L2).  P x is
 * formed by a scan of the structure, O(n nnz_p / 256) per thread: meant for the small dense P of the native QP path.
 * Enqueues two launches on `stream` (the test, then the count), allocates nothing, never synchronises the host; bracketed under profiling kind 2.
 * CE_E_TOO_LARGE when x, y, s and the three products of one instance exceed LDS.
 */
int ce_check_solved(ce_handle h, int B, const double *A_vals, long sA_k, long sA_b, const double *q_vals, long sq_k, long sq_b,
                    const double *P_vals, const int *p_rows, const int *p_cols, int nnz_p,
                    const double *x, const double *y, const double *s, const int *eligible /* NULL: all */, int eligible_mask,
                    double eps_abs, double eps_rel,
                    unsigned char *solved, int *status, int *iters, double *resid /* B x 3 */, int *n_unsolved, void *stream);

/* LPGD backward (Lagrangian proximal gradient descent, Paulus et al. 2024; diffcp's modes "lpgd", "lpgd_left", "lpgd_right").  The
 * gradient of a loss through the solution map is formed from one or two more solves of the SAME cone program with the cotangents added to its data, and a
 * difference of the Lagrangian's parameter gradient G = dL/dtheta (the envelope gradients of ce_value_vjp) at the solutions: no adjoint system, never rank
 * deficient.  For cotangents dx on x*, dy on y* (ds = 0), a step tau and a proximal weight rho >= 0 the perturbed program at +tau has
 *   c+ = c + tau dx - rho x*,   b+ = b - tau dy,   P+ = P + rho I,   A unchanged;          the one at -tau: the same call with -tau.
 *   lpgd_right: [G(x+, y+) - G(x*, y*)] / tau      lpgd_left: [G(x*, y*) - G(x-, y-)] / tau      lpgd: [G(x+, y+) - G(x-, y-)] / (2 tau)
 * The caller runs the solves itself (ce_solve / ce_solve_qp / ce_solve_shared_a on the outputs below, warm-started at the forward's point).  Both entry points
 * enqueue on `stream` only, never synchronise the host and allocate nothing; launches are bracketed under profiling kind 2.
 *   ce_lpgd_perturb : q_out (j, i) at [j*sq_k + i*sq_b] (q_vals' own strides) = fma(-rho, x[i, j], fma(tau, dx[i, j], q)) for j < n, the last row (d) copied.
 *                     dy [B][m] or NULL.  Given: A_out_bm [B][nnz_aug] becomes a copy of A_vals_bm (batch-major rows sA_b >= nnz_aug apart) in which the b
 *                     entry of row r alone moved by -tau dy[i, r] (the stored convention A_eval = [-A.data, b]); every other entry is bit-equal.  NULL: nothing
 *                     of A is read or written (A_vals_bm, A_out_bm may be NULL) -- solve on the forward's own values.
 *                     P_out [B][nnz_p] = P_vals + rho on the diagonal entries of the structure, written only when P_out is given, nnz_p > 0 and rho != 0.
 *                     flags [B]: bit 0 = every entry of dx and dy of the instance is exactly zero (its gradient is zero: skip it), bit 1 = some dy[i, r] != 0
 *                     sits on a row without a b entry in the template: that perturbation has no slot, it is dropped and reported here.
 *   ce_lpgd_grad    : from two points (x_a, y_a), (x_b, y_b) ([B][n], [B][m]) and the divisor delta (tau or 2 tau):  dA_vals (k, i) =
 *                     -(y_b,r Dx_c + Dy_r x_a,c) / delta (A entry) / -Dy_r / delta (b entry),  dq_vals (j, i) = Dx_j / delta, (n, i) = 0,
 *                     dP_vals[i, k] = (1/2 | 1) (x_b,r Dx_c + Dx_r x_a,c) / delta,  with Dx = x_b - x_a, Dy = y_b - y_a: the difference of two products is formed
 *                     from the differences of the points, never by cancelling the products.  Layouts, strides, NULL outputs, the P structure and skip as
 *                     ce_value_vjp: a skipped instance gets exact zeros whatever its inputs hold.  CE_E_TOO_LARGE when the points of four instances exceed LDS.
 * ce_set_transient_solve(h, 1): until switched off, ce_solve / ce_solve_qp on this handle leave no trace on it -- the batch-major inputs retained for
 * ce_vjp(A_vals = NULL) and the dispatch history (order, pending order, iteration memory) stay those of the last ordinary solve; A_vals must then be batch-major.
 * A solve issued from a backward pass runs under it, so a later adjoint or forward of another node sees what it would have seen without that backward. */
int ce_lpgd_perturb(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                    const double *P_vals, const int *p_rows, const int *p_cols, int nnz_p,
                    const double *x, const double *dx, const double *dy, double tau, double rho,
                    double *q_out, double *A_out_bm, double *P_out, int *flags, void *stream);
int ce_lpgd_grad(ce_handle h, int B, const double *x_a, const double *y_a, const double *x_b, const double *y_b, double delta, const unsigned char *skip,
                 double *dA_vals, long sdA_k, long sdA_b, double *dq_vals, long sdq_k, long sdq_b,
                 double *dP_vals, const int *p_rows, const int *p_cols, int nnz_p, void *stream);
int ce_set_transient_solve(ce_handle h, int on);

/* Longest-first dispatch.  Workgroups are dispatched in index order and one workgroup owns one instance, so the tail of a forward launch is set by the
 * instances that happen to start last: when they are long ones the last slots drain slowly (13 % of the metric configuration's kernel time).  With the switch
 * on, every ce_solve also records the order "instances by iteration count, largest first" (one tiny kernel behind the solve) and the NEXT ce_solve of the
 * same batch size dispatches its workgroups in that order -- PROVIDED the history has been predictive: the order is applied only when at least 70 % of the
 * instances of the last call stopped in the same check interval as the instance at the same position of the call before (decided on the device, no host
 * round trip).  Re-solved or slowly changing batches (full-batch training loops, parameter sweeps over a fixed data set) qualify from the third call on; on
 * unrelated batches (fresh mini-batches) the workgroups keep the index order, which is what is fastest there (a permutation that predicts nothing only scatters
 * the instances' rows over HBM: 1.5 % slower on the metric configuration).  A scheduling hint only: results are bit-identical in any order.
 * Register-tiled forward kernels only (fwd_mode 4).  Off by default at the C ABI. */
int ce_set_dispatch_history(ce_handle h, int on);

/* The LSQR re-solve of ce_vjp (see there): enable (default 1) and its stopping rule -- Paige & Saunders' atol / btol / conlim and the iteration limit
 * (0: diffcp's 2 (n + m + 1)); defaults = diffcp's adj_batch(mode="lsqr"): 1e-8, 1e-8, 1e8, 0.  <- diffcp_if.py:86. */
int ce_set_adjoint_resolve(ce_handle h, int enable, double atol, double btol, double conlim, int iter_lim);
/* >= 0: ce_vjp calls with the re-solve armed (q_vals given, enabled) run the SEARCH-FREE elimination kernel k_backward_ns (csrc/ce_backward_ns.h: the equality rows
 * are eliminated by one wave with column pivoting, the reduced Hessian on the null space is formed and swept on the matrix cores without a pivot search; a
 * vanishing pivot flags the instance for the LSQR re-solve) -- plain-cone templates with a linear objective and n <= 108; the value is the tile variant.
 * -1: the pivoting elimination kernels (k_backward_rt / k_backward) serve every call.  Introspection for tests / bench. */
int ce_adjoint_ns_variant(ce_handle h);

/* MANY COTANGENTS AT ONE SOLUTION: for every k < K what ce_vjp returns for (dx[k], dy[k]) under the same ce_set_adjoint_resolve rule, from ONE factorisation per
 * instance.  The matrix work of the search-free elimination (row-echelon form of the equality rows, null-space transform, reduced Hessian, blocked sweep) depends on
 * (A, x, y, s) alone; the sweep is an in-place inversion, so the kernel keeps (Z^T H Z)^-1 and B_1^-1 and rebuilds per cotangent only the classification-weighted
 * vectors, two short triangular replays, one product with the stored inverse and the dA row (csrc/ce_backward_ns.h, MANY).  A Jacobian of the solution map, several
 * loss heads on one layer and Gauss-Newton outer loops are K cotangents at one solution.
 *   A_vals_bm  batch-major rows, sA_b = nnz_aug apart (as ce_jvp takes them);  q_vals as ce_vjp (NULL: no re-solve, K plain ce_vjp calls inside)
 *   dx [K][B][n], dy [K][B][m] contiguous (dy NULL: zero);  dA_vals [K][B][nnz_aug] and dq_vals [K][B][n + 1] contiguous batch-major, boundary convention of ce_vjp;
 *   adj_status [K][B] (or NULL): the bit field of ce_vjp.  Rank deficiency is a property of the matrix: bits 4 and 8 are equal across k for an instance, which is
 *   listed for the LSQR re-solve once; one launch of the LSQR kernel serves all K cotangents of the listed instances.  Bit 1 is per cotangent.
 * K == 1 is legal.  CE_E_BADARG (before any device call): null handle or required pointer, B <= 0, K <= 0.  CE_E_UNSUPPORTED with a ce_last_error that names the reason
 * when ce_vjp_many_variant(h) < 0.  Batch-minor outputs are not served.  No host synchronisation, no allocation after the first call of a batch size. */
int ce_vjp_many(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                const double *x, const double *y, const double *s, const double *dx, const double *dy,
                double *dA_vals, double *dq_vals, int *adj_status, void *stream);
/* >= 0: the template has the many-cotangent mode; the value is the tile variant, ce_adjoint_ns_variant's (the mode rebuilds every cotangent's vectors in the plain
 * adjoint's buffers: same footprint, the launch plan is unchanged).  -1: PSD / exponential / power cones, a quadratic objective inside the kernels, n > 108,
 * CE_BWD_NS=0, or the LSQR vectors of the re-solve exceed LDS. */
int ce_vjp_many_variant(ce_handle h);

/* PARAMETER GRADIENTS STRAIGHT FROM THE ADJOINT'S FACTORS: what a caller with parameter maps wants from ce_vjp_many / ce_vjp is not dA (nnz_aug entries per pair) but
 * its product with the transposed maps.  Every dA entry is made of x, y and the adjoint's small solution (r_x, r_y, r_tau), so these entries keep the dA row out of
 * memory: the adjoint kernels store the factors per (cotangent, instance) pair and one streaming kernel (csrc/ce_param_grad.h) writes
 *     g[k][b][p] = sum_e val_e . dA_entry(i_e, j_e)  +  sum_e' val_e' . dq[j_e']          p = 0 .. rows - 1
 * for the map of the layer, COMPOSED by the caller once (cvxpylayers_amd/interfaces/param_grad.py): CSR over the rows (parameter columns, the constant column
 * included), the entries of the transposed A-map first and those of the transposed q-map behind them:
 *   map_ptr [rows + 1];  per entry  map_code, map_k (int), map_val (double):
 *     map_code >= 0: entry map_k of the value order, packed (i, j) = (map_code & 0xffff, map_code >> 16) -- its row and column, j == n: the b column
 *     map_code <  0: entry j = map_code & 0x7fffffff of dq (map_k unused)
 *   Every index must be in range (i < m, j <= n, map_k < nnz_aug): the library cannot check device arrays.
 * An entry is rounded as the dA entry first and multiplied by its value afterwards, in map order from a zero sum: a row with ONE entry has exactly the bits the dA
 * route gives; other rows agree within their terms' rounding.  Rows without an entry are written as 0.0.
 *   ce_vjp_many_params: ce_vjp_many's inputs (q_vals REQUIRED: the mode runs in front of the armed re-solve only) -> g [K][B][rows], dq_vals [K][B][n + 1],
 *                       adj_status [K][B] (required), all contiguous.  The elimination and the LSQR walk of the flagged instances store records instead of rows.
 *   ce_vjp_params     : one cotangent on the single-cotangent kernel (K = 1 of the many-mode is slower than ce_vjp): ce_vjp's inputs, g [B][rows], dq_vals with its
 *                       strides, adj_status [B] (required).  CE_E_UNSUPPORTED also when nnz_aug < m (the factors ride in the workspace row): use K = 1 above.
 *   ce_param_grad_variant: >= 0 exactly where ce_vjp_many_variant(h) >= 0 (the value is the same tile variant); -1: both entries return CE_E_UNSUPPORTED with a
 *                       ce_last_error that names the reason and write nothing.
 * CE_E_BADARG (before any device call): null handle or required pointer, B <= 0, K <= 0, rows <= 0.  No host synchronisation, no allocation after the first call
 * of a (B, K). */
int ce_vjp_many_params(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                       const double *x, const double *y, const double *s, const double *dx, const double *dy,
                       int rows, const int *map_ptr, const int *map_code, const int *map_k, const double *map_val,
                       double *g, double *dq_vals, int *adj_status, void *stream);
int ce_vjp_params(ce_handle h, int B, const double *A_vals, long sA_k, long sA_b, const double *q_vals, long sq_k, long sq_b,
                  const double *x, const double *y, const double *s, const double *dx, const double *dy,
                  int rows, const int *map_ptr, const int *map_code, const int *map_k, const double *map_val,
                  double *g, double *dq_vals, long sdq_k, long sdq_b, int *adj_status, void *stream);
int ce_param_grad_variant(ce_handle h);
/* Introspection (tests): the factor records the last ce_vjp_many_params call left in the engine's workspace, copied to out [K][B][m + 1 + n] on the stream: per pair
 * r_y[0 .. m), r_tau, r_x[0 .. n).  r_tau is 0 on the elimination path and LSQR's on a re-solved pair; g and dq do not determine it.  CE_E_STATE when no call of at
 * least this size has run. */
int ce_param_grad_records(ce_handle h, int B, int K, double *out, void *stream);

/* THE SAME FOR THE OTHER MANY-COTANGENT KINDS (additions under ABI 17).  Each entry is its kind's many-cotangent adjoint in record mode -- the record is the plain
 * kind's, r_y in the ORIGINAL basis (behind the triples' and the blocks' rotation), r_tau = 0 on the elimination path, r_x -- and k_param_grad behind it:
 *   ce_vjp_tri_many_params / ce_vjp_psd_many_params / ce_vjp_psd_tri_many_params: the arguments, layouts and rules of ce_vjp_many_params; served exactly where
 *       ce_vjp_tri_many_variant / ce_vjp_psd_many_variant / ce_vjp_psd_tri_many_variant (h) >= 0, with the re-solve armed (q_vals given).  A flagged instance is
 *       re-solved by LSQR per cotangent (4 | 8) and its records hold LSQR's (r_y, r_tau, r_x).
 *   ce_vjp_qp_many_params: ce_vjp_qp_many's inputs with the map and g in place of dA_vals / dP_vals; served where ce_vjp_qp_many_variant(h) >= 0.  Neither dA nor dP
 *       is written.  No re-solve: a rank-deficient instance keeps the dropped-variable answer with status 4, exactly as ce_vjp_qp_many.  The map may carry entries of dP:
 *         map_code < 0 with bit 30 CLEAR: entry j = map_code & 0x3fffffff of dq (as above: n < 2^15)
 *         map_code < 0 with bit 30 SET  : entry map_k of P's structure order, packed (i, j) = (map_code & 0x7fff, map_code >> 15 & 0x7fff): the value is ONE share
 *                                         -1/2 (r_x,i x_j + r_x,j x_i); ce_vjp_qp_many's doubling of a one-triangle entry with i != j (and a frontend's symmetrisation)
 *                                         belongs in map_val.  Per row the P entries stand behind the q entries.
 * Every entry refuses a handle of another kind with CE_E_UNSUPPORTED before anything is enqueued and writes nothing; ce_vjp_many_params, ce_vjp_params and
 * ce_param_grad_variant keep refusing every handle that is not plain.  ce_param_grad_records serves the last call of any kind. */
int ce_vjp_tri_many_params(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                           const double *x, const double *y, const double *s, const double *dx, const double *dy,
                           int rows, const int *map_ptr, const int *map_code, const int *map_k, const double *map_val,
                           double *g, double *dq_vals, int *adj_status, void *stream);
int ce_vjp_psd_many_params(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                           const double *x, const double *y, const double *s, const double *dx, const double *dy,
                           int rows, const int *map_ptr, const int *map_code, const int *map_k, const double *map_val,
                           double *g, double *dq_vals, int *adj_status, void *stream);
int ce_vjp_psd_tri_many_params(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                               const double *x, const double *y, const double *s, const double *dx, const double *dy,
                               int rows, const int *map_ptr, const int *map_code, const int *map_k, const double *map_val,
                               double *g, double *dq_vals, int *adj_status, void *stream);
int ce_vjp_qp_many_params(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *P_vals, const double *x, const double *y, const double *s,
                          const double *dx, const double *dy, int rows, const int *map_ptr, const int *map_code, const int *map_k, const double *map_val,
                          double *g, double *dq_vals, int *adj_status, void *stream);

/* MANY TANGENTS AT ONE SOLUTION: for every k < K what ce_jvp (ce_jvp_qp) returns for the k-th tangent, from ONE factorisation per instance -- the forward twin of
 * ce_vjp_many, and the route by which a layer with few parameters and many outputs, or a native QP layer, gets its Jacobian by columns.  The matrix work is the
 * adjoint's and depends on (A, x, y, s [, P]) alone; per tangent the kernel rebuilds g = dQ pi from the tangent's rows and the point (read from global memory again),
 * gamma and the weights of f from the retained classification, d~ from the in-place B_1^-1, the reduced right-hand side, one product with the stored
 * (Z^T (H [+ P]) Z)^-1, step 5 and the forward epilogue (csrc/ce_backward_ns.h, FWD + MANY).
 *   A_vals_bm, q_vals, P_vals, x, y, s, atol .. iter_lim as ce_jvp / ce_jvp_qp.
 *   tangent k of instance i:  its value row at tA_vals + k * stA_k + i * stA_b,  its q_eval row (n + 1 CONTIGUOUS entries, the last ignored) at
 *   tq_vals + k * stq_k + i * stq_b,  its P row at tP_vals + k * stP_k + i * stP_b.  Each pointer may be NULL (zero).  A batch stride is 0 -- one row shared by
 *   every instance: a parameter-space basis vector pushed through the parameter maps -- or at least the row length; anything between is CE_E_BADARG.
 *   dx [K][B][n], dy [K][B][m], ds [K][B][m] (ds may be NULL), jvp_status [K][B], lsqr_iters [K][B] (may be NULL) contiguous.
 * Rank deficiency is the matrix's: ce_jvp_many flags such an instance for all K, lists it once, and one launch of the LSQR kernel serves all K tangents of the listed instances (status 4 | 8,
 * iterations > 0, as ce_jvp); ce_jvp_qp_many has no re-solve, the dropped-variable answer stands with status 4 for every k (as ce_jvp_qp).
 * K == 1 is legal.  CE_E_BADARG (before any device call): null handle or required pointer, B <= 0, K <= 0, a bad batch stride.  CE_E_UNSUPPORTED with a
 * ce_last_error that names the reason when the kind's *_many_variant is -1.  No host synchronisation, no allocation after the first call of a batch size. */
int ce_jvp_many(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                const double *x, const double *y, const double *s,
                const double *tA_vals, long stA_k, long stA_b, const double *tq_vals, long stq_k, long stq_b,
                double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters,
                double atol, double btol, double conlim, int iter_lim, void *stream);
int ce_jvp_qp_many(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *P_vals,
                   const double *x, const double *y, const double *s,
                   const double *tA_vals, long stA_k, long stA_b, const double *tq_vals, long stq_k, long stq_b, const double *tP_vals, long stP_k, long stP_b,
                   double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters, void *stream);
/* >= 0: the template has the many-tangent mode of its kind; the value is the tile variant (ce_adjoint_ns_variant's / ce_qp_ns_variant's: the mode rebuilds every
 * tangent's vectors in the buffers of ce_jvp / ce_jvp_qp, the launch plan is unchanged).  -1: no in-kernel mode -- PSD / exponential / power cones (triples have
 * ce_jvp_tri_many), n > 108, CE_BWD_NS=0, the LSQR vectors of the re-solve exceed LDS, the other kind's template; a NULL handle. */
int ce_jvp_many_variant(ce_handle h);
int ce_jvp_qp_many_variant(ce_handle h);

/* MANY COTANGENTS AT ONE SOLUTION, QUADRATIC OBJECTIVE INSIDE THE KERNELS: for every k < K what ce_vjp_qp returns for (dx[k], dy[k]) on a QP-native template, dP
 * included, from ONE factorisation per instance by the search-free elimination -- the reverse twin of ce_jvp_qp_many.  The system is (H + P) r_x - B^T mu = f,
 * B r_x = d_B; steps 1-4 with P (its rows through the null-space transform, Z^T P Z on the matrix cores) depend on (A, P, x, y, s) alone, and per cotangent the kernel
 * rebuilds what ce_vjp_many rebuilds plus the P terms (t_j = p_j . x_p and Z^T P x_p in the reduced right-hand side, (P r_x)[piv] for the multipliers), then writes
 * the dA row, dq and dP = -sym(r_x x^T) through the structure of P, a one-triangle entry doubled (csrc/ce_backward_ns.h, QP + MANY without FWD).
 *   A_vals_bm  batch-major rows, sA_b = nnz_aug apart;  P_vals [B][nnz_p];  dx [K][B][n], dy [K][B][m] contiguous (dy NULL: zero);
 *   dA_vals [K][B][nnz_aug], dq_vals [K][B][n + 1] as ce_vjp_many;  dP_vals [K][B][nnz_p];  adj_status [K][B] (or NULL).
 * Rank deficiency is the matrix's: a vanishing pivot drops the variable, the instance gets status 4 for every k and keeps the finite dropped-variable answer.  There is
 * no LSQR re-solve (no LSQR has a P term): bit 8 is never set.  ce_vjp_qp's pivoting kernel treats such an instance differently (its own basic solution).
 * K == 1 is legal.  CE_E_BADARG (before any device call): null handle or required pointer, B <= 0, K <= 0, non-contiguous A rows.  CE_E_UNSUPPORTED with a
 * ce_last_error that names the reason when ce_vjp_qp_many_variant(h) < 0.  No host synchronisation, no allocation after the first call of a batch size.
 * ce_vjp_many keeps refusing QP-native templates. */
int ce_vjp_qp_many(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *P_vals,
                   const double *x, const double *y, const double *s, const double *dx, const double *dy,
                   double *dA_vals, double *dq_vals, double *dP_vals, int *adj_status, void *stream);
/* >= 0: the template runs a quadratic objective inside the kernels and has the search-free elimination with P; the value is ce_qp_ns_variant's row (same
 * footprint, the launch plan is unchanged).  -1 otherwise, and for a NULL handle. */
int ce_vjp_qp_many_variant(ce_handle h);

/* MANY COTANGENTS AT ONE SOLUTION, EXPONENTIAL / POWER CONES: for every k < K what ce_vjp returns for (dx[k], dy[k]) on a template with exponential or 3-d power
 * triples beside plain cones (linear objective, no PSD block), from ONE factorisation per instance by the search-free elimination -- where ce_vjp runs the pivoting
 * kernel once per cotangent.  Once per instance D Pi of every triple is diagonalised, W diag(lambda) W^T, its three rows of A are rotated (a rotated row is an
 * equality, a dropped row or one weighted row of the reduced Hessian) and steps 1-4 run on a zero right-hand side; per cotangent the kernel rebuilds what ce_vjp_many
 * rebuilds plus h = W^T dy_c per triple (d_B entry, 0, or d = lambda h with the share theta h of f), and rotates r_y back, r_y,c = W r~_y,c, in front of the dA row
 * (csrc/ce_backward_ns.h, TRI + MANY without FWD).
 *   Arguments, layouts, dy == NULL, K == 1, q_vals == NULL / a switched-off re-solve (K ce_vjp calls inside) and the error rules are exactly ce_vjp_many's.
 * Flags belong to the matrix: a vanishing pivot, more active rows than variables, or a weighted triple row with 1 - lambda < 1e-5 (the forward derivative's rule
 * for a stiff row, carried over) flag the instance for every k; it is listed once and one launch of the LSQR kernel serves all K cotangents of the listed instances (status 4 | 8).  The
 * pivoting kernel behind ce_vjp need not flag the same instances: a flagged instance gets LSQR's minimum-norm answer.
 * CE_E_UNSUPPORTED with a ce_last_error that names the reason when ce_vjp_tri_many_variant(h) < 0.  ce_vjp_many keeps refusing such templates. */
int ce_vjp_tri_many(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                    const double *x, const double *y, const double *s, const double *dx, const double *dy,
                    double *dA_vals, double *dq_vals, int *adj_status, void *stream);
/* >= 0: the template has the many-cotangent mode with triples; the value is ce_tri_ns_variant's row (same footprint, the launch plan is unchanged).  -1 otherwise,
 * and for a NULL handle. */
int ce_vjp_tri_many_variant(ce_handle h);

/* MANY TANGENTS AT ONE SOLUTION, EXPONENTIAL / POWER CONES: for every k < K what ce_jvp returns for the k-th tangent on a template with exponential or 3-d power
 * triples beside plain cones (linear objective, no PSD block), from ONE factorisation per instance -- the forward twin of ce_vjp_tri_many, where ce_jvp
 * re-diagonalises every triple, re-rotates its rows and re-factors every instance once per tangent.  Once per instance D Pi of every triple is diagonalised,
 * W diag(lambda) W^T (lambda snapped to 0 / 1 within 1e-9), its three rows of A are rotated and steps 1-4 run on a zero right-hand side; per tangent the kernel
 * rebuilds what ce_jvp_many rebuilds plus gamma_c = W^T g_y,c per triple (a lambda = 1 row: its entry of d_B; a lambda = 0 row: nothing; a weighted row: theta gamma
 * in f and theta t in the list), then step 5 and the triples' forward epilogue, dy = W lambda eta, ds = -W (1 - lambda) eta (csrc/ce_backward_ns.h, FWD + TRI + MANY).
 *   Arguments, layouts, strides (a batch stride of 0: one tangent row for the whole batch), K == 1 and the error rules are exactly ce_jvp_many's.
 * Flags belong to the matrix: a vanishing pivot, more active rows than variables, or a weighted triple row with 1 - lambda < 1e-5 (ce_jvp's own rule for a stiff
 * row) flag the instance for every k; it is listed once and ONE launch of the LSQR kernel re-solves all K tangents of the listed instances (status 4 | 8,
 * iterations > 0, the answers of K ce_jvp calls bit for bit).
 * CE_E_UNSUPPORTED with a ce_last_error that names the entry point and the reason when ce_jvp_tri_many_variant(h) < 0; nothing is written then.  ce_jvp_many keeps
 * refusing templates with triples. */
int ce_jvp_tri_many(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                    const double *x, const double *y, const double *s,
                    const double *tA_vals, long stA_k, long stA_b, const double *tq_vals, long stq_k, long stq_b,
                    double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters,
                    double atol, double btol, double conlim, int iter_lim, void *stream);
/* >= 0: the template has the many-tangent mode with triples; the value is ce_tri_ns_variant's row (the rebuild lives in the buffers of the triples' footprint: no
 * shape is excluded, the launch plan is unchanged).  -1 otherwise, and for a NULL handle. */
int ce_jvp_tri_many_variant(ce_handle h);

/* MANY COTANGENTS AT ONE SOLUTION, PSD BLOCKS: for every k < K what ce_vjp returns for (dx[k], dy[k]) on a template with PSD blocks beside plain cones (linear
 * objective, no exponential / power cone), from ONE factorisation per instance by the search-free elimination -- where ce_vjp runs the pivoting kernel, and with it
 * the blocks' Jacobi decompositions, once per cotangent.  Once per instance smat(v_c) = U Lambda U^T of every block, its rows of A are rotated into the basis in
 * which D Pi is diagonal with eigenvalue B (a rotated row is an equality, a dropped row or one weighted row of the reduced Hessian) and steps 1-4 run on a zero
 * right-hand side; per cotangent the kernel rebuilds what ce_vjp_many rebuilds plus h = Q^T dy_c per block (d_B entry, 0, or d = B h with the share theta h of f),
 * and rotates r_y back, r_y,c = Q r~_y,c, in front of the dA row (csrc/ce_backward_ns.h, MANY + PSD without FWD).
 *   Arguments, layouts, dy == NULL, K == 1, q_vals == NULL / a switched-off re-solve (K ce_vjp calls inside) and the error rules are exactly ce_vjp_many's.
 * Flags belong to the matrix: a vanishing pivot, more active rows than variables, or a weighted PSD row with 1 - B < 1e-5 (the forward derivative's rule for a stiff
 * row of a triple, carried over again: not measured on PSD rows) flag the instance for every k; it is listed once and one launch of the LSQR kernel serves all K
 * cotangents of the listed instances (status 4 | 8).  The pivoting kernel behind ce_vjp need not flag the same instances.
 * CE_E_UNSUPPORTED with a ce_last_error that names the reason when ce_vjp_psd_many_variant(h) < 0.  ce_vjp_many and ce_vjp_tri_many keep refusing such templates. */
int ce_vjp_psd_many(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                    const double *x, const double *y, const double *s, const double *dx, const double *dy,
                    double *dA_vals, double *dq_vals, int *adj_status, void *stream);
/* >= 0: the template has the many-cotangent mode with PSD blocks; the value is ce_psd_ns_variant's row (same footprint, the launch plan is unchanged).  -1
 * otherwise, and for a NULL handle. */
int ce_vjp_psd_many_variant(ce_handle h);

/* MANY TANGENTS AT ONE SOLUTION, PSD BLOCKS: for every k < K what ce_jvp_psd returns for the k-th tangent, from ONE factorisation per instance -- the forward twin of
 * ce_vjp_psd_many, where ce_jvp_psd re-decomposes every block, re-rotates its rows and re-factors every instance once per tangent.  Per tangent the kernel rebuilds
 * what ce_jvp_many rebuilds plus gamma_c = Q^T g_y,c per block (a B = 1 row: its entry of d_B; a B = 0 row: nothing; a weighted row: theta gamma in f and theta t in
 * the list), then step 5 and the blocks' forward epilogue, dy_c = Q (B o eta), ds_c = -Q ((1 - B) o eta) (csrc/ce_backward_ns.h, FWD + MANY + PSD).
 *   Arguments, layouts, strides (a batch stride of 0: one tangent row for the whole batch), K == 1 and the error rules are exactly ce_jvp_many's.
 * Flags as ce_vjp_psd_many (ce_jvp_psd's own rule for a stiff row); a flagged instance is listed once and ONE launch of the LSQR kernel re-solves all K tangents of
 * the listed instances (status 4 | 8, iterations > 0, the answers of K ce_jvp_lsqr calls on those instances).
 * CE_E_UNSUPPORTED with a ce_last_error that names the entry point and the reason when ce_jvp_psd_many_variant(h) < 0; nothing is written then.  ce_jvp_many and
 * ce_jvp_tri_many keep refusing templates with PSD blocks. */
int ce_jvp_psd_many(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                    const double *x, const double *y, const double *s,
                    const double *tA_vals, long stA_k, long stA_b, const double *tq_vals, long stq_k, long stq_b,
                    double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters,
                    double atol, double btol, double conlim, int iter_lim, void *stream);
/* >= 0: the template has the many-tangent mode with PSD blocks; the value is ce_psd_ns_variant's row.  -1 otherwise, and for a NULL handle. */
int ce_jvp_psd_many_variant(ce_handle h);

/* PSD BLOCKS AND EXPONENTIAL / POWER TRIPLES IN ONE TEMPLATE (log_det and its kin: one PSD block beside one exponential cone per diagonal entry): the four
 * search-free modes on a template with both cone kinds beside plain cones, linear objective.  Per instance the kernel does what the two kinds do on their own, in
 * sequence: each triple's D Pi is diagonalised, snapped, and its three rows of A rotated; each block is Jacobi-decomposed and its rows rotated; every rotated row is
 * an equality, a dropped row or one weighted row; steps 1-4; both epilogues, both rotations back (csrc/ce_backward_ns.h, TRI + PSD).  Entry points of their own, each
 * with the arguments, layouts, strides, statuses and error rules of its PSD sibling:
 *   ce_jvp_psd_tri       as ce_jvp_psd       (one tangent; flagged instances re-solved by LSQR behind it, status 4 | 8)
 *   ce_refine_psd_tri    as ce_refine_psd    (safeguarded Newton steps, the PSD kind's shortened steps 1/2, 1/4, 1/8; y-hat of a triple from its cold-start decision
 *                                             and y-hat of a block from its decomposition inside one acceptance test)
 *   ce_vjp_psd_tri_many  as ce_vjp_psd_many  (K cotangents on one factorisation; per cotangent h = W^T dy_c per triple and h = Q^T dy_c per block)
 *   ce_jvp_psd_tri_many  as ce_jvp_psd_many  (K tangents on one factorisation; per tangent gamma_c = W^T g_y,c per triple and gamma_c = Q^T g_y,c per block)
 * Flags (status 4 | 8 behind the re-solve): a vanishing pivot, more active rows than variables, or a weighted triple OR PSD row with 1 - lambda < 1e-5 -- the forward
 * derivative's measured rule for a stiff row of a triple, carried over again to the mixed kind: not measured on PSD rows, not measured for an adjoint.  A flagged
 * instance is listed once, and in the many-modes ONE launch of the LSQR kernel serves all K right-hand sides.  The refinement flags no stiff row.
 *   ce_psd_tri_ns_variant: the row of the kernel's variant list the four modes run on (>= 0: a PSD block and a triple, no quadratic objective, n <= 108, the footprint
 * with both kinds' segments on top fits LDS, and the LSQR vectors of the re-solve fit LDS); -1: none, or h == NULL.  ce_psd_tri_ns_lds: that footprint in bytes
 * (0 when there is none).  ce_vjp_psd_tri_many_variant / ce_jvp_psd_tri_many_variant: the same row, or -1.
 *   CE_E_UNSUPPORTED with a ce_last_error that names the entry point and the reason when the variant is < 0; nothing is written then.  ce_jvp, ce_refine, ce_jvp_psd,
 * ce_refine_psd, ce_vjp_many, ce_jvp_many, ce_vjp_tri_many, ce_jvp_tri_many, ce_vjp_psd_many and ce_jvp_psd_many keep refusing such templates; ce_get_plan keeps its
 * 18 entries. */
int ce_jvp_psd_tri(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                   const double *x, const double *y, const double *s, const double *tA_vals_bm, long stA_b, const double *tq_vals, long stq_k, long stq_b,
                   double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream);
int ce_refine_psd_tri(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b, double *x, double *y, double *s,
                      const int *status, int steps, int *refine_status, int *steps_taken, double *resid, void *stream);
int ce_vjp_psd_tri_many(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                        const double *x, const double *y, const double *s, const double *dx, const double *dy,
                        double *dA_vals, double *dq_vals, int *adj_status, void *stream);
int ce_jvp_psd_tri_many(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                        const double *x, const double *y, const double *s,
                        const double *tA_vals, long stA_k, long stA_b, const double *tq_vals, long stq_k, long stq_b,
                        double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters,
                        double atol, double btol, double conlim, int iter_lim, void *stream);
int ce_psd_tri_ns_variant(ce_handle h);
long ce_psd_tri_ns_lds(ce_handle h);
int ce_vjp_psd_tri_many_variant(ce_handle h);
int ce_jvp_psd_tri_many_variant(ce_handle h);

/* Introspection used by bench.py / tests: per-kernel HIP-event timing on the launch stream.  enable: 0 off, 1 every launch, or a sum of 2 (forward launches),
 * 4 (adjoint launches), 8 (layout passes) to bracket only those kinds (two event records per bracketed launch are host work in front of the launch). */
int ce_set_profiling(ce_handle h, int enable);
/* which: 0 forward kernel, 1 backward kernel, 2 layout (transpose) kernels and the streaming passes of ce_value / ce_value_jvp / ce_value_vjp.  Returns the mean ms per launch
 * since the last ce_reset_profile and the launch count; synchronises the recorded events. */
int ce_get_profile(ce_handle h, int which, double *mean_ms, int *launches);
int ce_reset_profile(ce_handle h);
/* LDS bytes per workgroup and residency mode chosen for (forward, backward); for DESIGN/bench reporting.
 * fwd_mode: 0..2 size-generic kernel (everything in LDS / G in global memory / A and G in global memory), 3 k_forward_rt, 4 k_fwd2 (register tiles,
 * LDS operand streams).
 * bwd_mode: 0..2 size-generic kernel, 3 k_backward_rt. */
int ce_get_launch_info(ce_handle h, int *fwd_lds_bytes, int *bwd_lds_bytes, int *fwd_mode, int *bwd_mode);
/* The whole launch plan of the handle, for tests: writes min(n_out, count) ints to out (may be NULL) and returns count (CE_E_BADARG for a null handle).
 * Order (fixed; later ABI versions only append):
 *    0 fwd_mode       as ce_get_launch_info
 *    1 f2_variant     k_fwd2 register-tile variant 0..4 (-1: not k_fwd2)
 *    2 rt_variant     k_forward_rt variant 0..2 (-1: none; k_fwd2 may serve the template while this is set)
 *    3 wl             1: k_fwd2 rows packed so that every cone is wave-local
 *    4 aa_ok          1: k_fwd2 carries the Anderson-acceleration vectors in LDS
 *    5 gen_blocked_f  1: the size-generic forward inverts its global-memory G by column panels
 *    6 qp_native      1: the quadratic objective runs inside the kernels
 *    7 bwd_mode       as ce_get_launch_info
 *    8 brt_variant    k_backward_rt variant 0..6 (-1: none)
 *    9 two_tile       1: calls with adj_status run the two-tile plan of k_backward_rt
 *   10 ns_variant     as ce_adjoint_ns_variant
 *   11 gen_blocked_b  1: the size-generic backward eliminates its global-memory K by column panels
 *   12 sp_r           dense rows (two or more entries) of the A part, when at most 64 (shared-A kernels; else 0)
 *   13 sp_RP          their padding 16 / 32 / 64 (0: more than 64 dense rows, the batch-GEMM path of the constant-A interface)
 *   14 last_fast      first tile of the last ce_vjp call when it ran the two-tile plan (-1: the call ran one tile / none yet)
 *   15 last_sa_fwd    row of CE_SA_FWD_VARIANTS (csrc/ce_variants.h) the last ce_solve_shared_a call launched (-1: none yet)
 *   16 last_sa_lsqr   row of CE_SA_LSQR_VARIANTS the last k_sa_lsqr launch ran: ce_vjp_shared_a, ce_vjp_lsqr, ce_jvp_shared_a, ce_jvp_lsqr, or the re-solve behind
 *                     ce_vjp / ce_jvp (-1: none yet)
 *   17 tri_ns_variant as ce_tri_ns_variant
 * The plan is fixed by ce_create (environment switches included), except the last_* entries: the shared-A kernels read their switches at the call. */
int ce_get_plan(ce_handle h, int *out, int n_out);

/* ---- The projection onto a product of cones and its derivative as an operation of its own (diffcp's cones.pi / cones.dpi) ----
 * A projection needs no template matrix, so it has a light handle of its own: the cone layout (offsets, orders, exponents), uploaded once.  Rows in the solver's
 * order z, l, q, s, ep, p; PSD blocks as svec (lower triangle, column-major, sqrt(2) off-diagonals); a negative power-cone entry -a is the dual cone of exponent a.
 *   ce_cones_create   : validates on the host and checks the LDS footprint of every PSD order BEFORE any HIP call: CE_E_TOO_LARGE for an order above 82
 *                       (csrc/ce_lds_cone_proj.h; ce_last_error names the order and the bound), CE_E_BADARG for a malformed description.
 *   ce_cones_rows     : m, the rows of the set.
 *   ce_cones_state_len: doubles of derivative state per instance: k^2 + k per PSD block (eigenvectors, unclipped eigenvalues) + 9 per exponential / power triple
 *                       (its Jacobian).  Zero / nonnegative / second-order cones keep none.
 *   ce_cone_project   : out = Pi_K(v), or Pi_K*(v) for dual != 0 (the zero cone projects to 0, its dual is free; every other dual is the true dual cone).  v and out
 *                       are (B, m) with row pitches ld_v, ld_out >= m in elements; out must not alias v.  state (B, ce_cones_state_len) or NULL: not wanted, nothing
 *                       of the derivative is then computed.  A non-finite entry makes the rows of ITS cone NaN and touches nothing else.
 *   ce_cone_dproject  : out = D Pi(v) dir for the same v, dual, and the state that call wrote (may be NULL when ce_cones_state_len is 0).  D Pi is symmetric for
 *                       every kind, so this one call is both the forward- and the reverse-mode derivative.  Conventions at kinks: a nonnegative row at exactly 0 has
 *                       factor 1/2; a second-order cone is the identity on the cone's boundary and 0 on the polar's; PSD divided differences are 1 for two positive
 *                       eigenvalues, 0 for two non-positive ones.
 * One launch per cone kind present (rows and second-order cones share one); the calls only enqueue. */
typedef struct ce_cones *ce_cones_handle;
int ce_cones_create(int z, int l, int nq, const int *q, int ns, const int *s, int nep, int np, const double *p, int device, ce_cones_handle *out);
int ce_cones_destroy(ce_cones_handle h);
int ce_cones_rows(ce_cones_handle h);
long ce_cones_state_len(ce_cones_handle h);
int ce_cone_project(ce_cones_handle h, int B, const double *v, long ld_v, int dual, double *out, long ld_out, double *state, void *stream);
int ce_cone_dproject(ce_cones_handle h, int B, const double *v, long ld_v, int dual, const double *state, const double *dir, long ld_dir,
                     double *out, long ld_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CONE_ENGINE_H */

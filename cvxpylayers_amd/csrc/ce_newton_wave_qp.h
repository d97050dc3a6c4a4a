// ce_newton_wave_qp.h -- k_newton_wave_qp: the forward derivative and one Newton refinement step of a SMALL template with a QUADRATIC objective inside the kernels,
// one instance per wave (opt-in: ce_jvp_qp_wave, ce_refine_qp_wave).
//
// The system and the answers are k_backward_ns<..., FWD, QP> / <..., FWD, REF, QP>'s (ce_backward_ns.h).  With d_tau pinned to 0 the forward block
//        P d_x + A^T D d_y = -g_x,    -A d_x + (I - D) d_y = -g_y            (A in the solver form stored here, A = -A_cvx)
// reduces in the eigenbasis of D per cone (eta = W^T d_y, gamma = W^T g_y) to
//        (H + P) d_x + B^T eta_B = f = -g_x + sum theta a~^T gamma,   B d_x = gamma_B,        H = sum_c theta_c (A_z^T A_z - a_z a_z^T),  B = the neq equality rows.
// It is k_newton_wave (ce_newton_wave.h) -- its prologues, classification, kink rules, stages 1-5, eta epilogue, safeguard and record -- with P added the way
// k_bwd_wave_qp (ce_backward_wave_qp.h) adds it to k_bwd_wave.  Both are RESTATED here, not shared through helpers: newton_wave.o's and bwd_wave_qp.o's device code
// stay byte-identical, and a restated kernel cannot touch them.  What P adds:
//   load      P is a third dense LDS matrix (n rows of NX + 1) behind A and R | B_1^-1, zeroed with them, scattered from the instance's row of P_vals through the
//             handle's (row, column) arrays: a one-triangle entry fills (i, j) and (j, i), a full-structure entry its own slot (k_fwd_wave_qp's convention).
//   REF = false  g_x = tq - tA^T y + tP x: the tangent's P row is read ONCE and scattered dense into the buffer P takes afterwards (entry (i, j) of the structure
//             into slot [j][i], so that one wv_mv_cols over the buffer is row i of tP against x: k_backward_ns<FWD, QP>'s product, whatever the symmetry of
//             the tangent's values), beside the tangent's value row in the buffer A takes afterwards; then the three buffers are cleared and A and P loaded.
//             Each of tA, tq, tP may be NULL: zero.
//   REF = true   F_x = P x + A^T y^ + c: one more wv_mv_cols over the P buffer in the residual; rho = max |F| / (1 + max(|b|, |c|)), k_backward_ns<REF, QP>'s
//             normalisation (P does not enter the scale).  The elimination overwrites P in place, so the epilogue scatters P again beside the value row before rho+.
//   stage 2   while the eliminated rows c1[] are registers: every row of P through transform() (W = P Z in the free columns, the pivot columns keep P), then every
//             FREE column b of W, read with lane = row, through the same transform(): column b of Z^T P Z, by symmetry its row b with lane = column, and lane n
//             ends with -(Z^T P x_p)_b on its own.  Written back in place (free rows of column b; column NX of row b): c1[] and G[] are never live together.
//   stage 3   G[a] starts from row a of that buffer (lane n: -(Z^T P x_p)_a), the Gram of H's weighted rows is accumulated onto it; dg, the diagonal the sweep's
//             rank test compares against, is Z^T (H + P) Z's.  No weighted row and neq = 0: the reduced Hessian is P alone.
//   stage 5   g = ((H + P) d_x - f)[piv]: (P d_x)[p_e] is one more wv_mv_cols over the P buffer with the staged d_x -- pivot columns untouched, P symmetric.
//   flags     k_backward_ns<FWD, QP>'s: neq > n is status 4 (forward derivative: zero outputs; refinement: bit 4, the point kept); a dropped equality row or variable
//             sets bit 4 and the forward derivative's dropped-variable answer stands, finite.  No re-solve list, no LSQR (none has a P term): bit 8 is never set.
//
// Rules restated from k_backward_ns and k_newton_wave (the kernels must decide alike):
//   rows       zero rows are equalities; a nonnegative row is an equality when v = y - s > 0, else eliminated (lambda = 0: eta = a . d_x - gamma from its untouched row).
//   cones      v = (t0, z), nz = |z|, dimension d:  d == 1: inside when t0 >= 0, else polar;  nz <= t0: inside (every row an equality);  nz <= -t0: polar (every row
//              eliminated);  else boundary, lam = (t0 + nz) / (2 nz), theta = lam / (1 - lam): one equality e_y with gamma_y = (g_0 + z-hat . g_z) / sqrt 2 (written
//              over the cone's t-row), the z-rows weighted theta in H and a_z = A_z^T z-hat weighted -theta; the rows' weights in f are
//              u_i = theta (g_i - z-hat_i (z-hat . g_z)), 0 on the t-row.  y^ = v inside, 0 in the polar, lam (nz, z) on the boundary.
//   record     REF: status bits 1 kept / 2 rejected / 4 flagged / 16 skipped, steps, resid are ce_refine_qp's; the step is kept only when rho+ is below rho as evaluated
//              now AND as recorded.  A rejected, flagged or skipped instance keeps its point bit for bit.
//
// Placement: k_newton_wave's.  Lane i < m owns cone row i, lane j < n variable j, lane n the right-hand side of the register rows; A (m rows of NX + 1), R | B_1^-1
// (NX rows of NX + 1) and P (n rows of NX + 1) in this wave's LDS, the equality rows and then the rows of the reduced Hessian NX registers per lane.  The carve is
// k_bwd_wave_qp's to the byte: the prologues stage b (and the tangent's b entries) in the R buffer, which is idle until a_z.
// LDS is written and read by the owning wave only: wv_sync() orders the accesses, no workgroup barrier.  Every loop is bounded by n, m, neq, nnz, nnz_p, the number
// of cones or a compile-time count.
#pragma once
#include "ce_common.h"
#include "ce_wave_helpers.h"
#include "ce_forward_wave.h"        // wv_sync, fold, lane_bcast, wv_max, wv_mv_cols, wv_mv_rows: the one-wave building blocks
#include "ce_backward_wave.h"       // lane_bcast_i, bw_recip
#include "ce_lds_newton_wave_qp.h"  // newton_wave_qp_lds_doubles: the total of the carve below

template <bool REF> struct NewtonWaveQpArg { typedef NsJvp type; };
template <> struct NewtonWaveQpArg<true> { typedef NsRefine type; };

template <int NX, int MY, int WPS, bool REF>
__global__ void __launch_bounds__(64, WPS)
k_newton_wave_qp(DevT T, const double *__restrict__ Avals, NwQp Q, const double *xg, const double *yg, const double *sg, int *__restrict__ adj_status,
                 typename NewtonWaveQpArg<REF>::type W) {
    static_assert(NX <= 32 && MY <= 64 && 64 % NX == 0 && 64 % MY == 0 && NX >= 8 && NX < MY, "k_newton_wave_qp: one lane per row, one per column and one for the right-hand side");
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int LD = NX + 1, NG = NX / 8;
    const int lane = threadIdx.x;
    const size_t inst = blockIdx.x;
    const int n = T.n, m = T.m, z = T.z, zl = T.z + T.l, nq = T.nq, nnz = T.nnz_aug, nnz_p = Q.nnz_p;
    double *A = sm, *Rp = A + m * LD, *Pm = Rp + NX * LD, *xb = Pm + n * LD, *xb2 = xb + NX, *yb = xb2 + NX, *yb2 = yb + MY;
    int *erow = (int *)(yb2 + MY);
    const bool xm = lane < n, ym = lane < m;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const double *const vals = Avals + inst * nnz;
    const double *const pvals = Q.P + inst * (size_t)nnz_p;

    // ---------------------------------------------------------------- REF: the instance's record of this call (ce_refine_qp's rules)
    int rst0 = 0; double rho_cur = 0.0, rho0 = 0.0;
    if constexpr (REF) {
        rst0 = __builtin_amdgcn_readfirstlane(W.first ? ((W.status && W.status[inst] < 0) ? 16 : 0) : W.rstatus[inst]);      // (wave-uniform: scalar registers)
        if (!W.first) rho_cur = uniform_d(W.resid[2 * inst + 1]);
        if (W.first && lane == 0) {
            W.rstatus[inst] = rst0; W.steps[inst] = 0;
            if (rst0) { W.resid[2 * inst] = __builtin_nan(""); W.resid[2 * inst + 1] = __builtin_nan(""); }
        }
        if (rst0 & (2 | 4 | 16)) return;
    }

    int qe = 0;      // first row behind the second-order cone this lane's row belongs to (k_fwd_wave's walk)
    if (ym && lane >= zl) qe = T.qoff[T.rowcone[lane] + 1];
    auto for_cones = [&](auto &&f) {
        int r0 = zl;
        for (int c = 0; c < nq; c++) { const int r1 = __builtin_amdgcn_readlane(qe, r0); f(r0, r1); r0 = r1; }
    };
    auto stage_x = [&](double *buf, double v) { if (lane < NX) buf[lane] = v; };
    auto stage_y = [&](double *buf, double v) { if (lane < MY) buf[lane] = v; };
    auto clear_all = [&]() { for (int i = lane; i < (m + NX + n) * LD; i += 64) A[i] = 0.0; };      // (A, R and P are contiguous)
    // A = -A_cvx dense through the template's structure; REF: b (column n of the value row) into the head of the R buffer
    auto load_A = [&]() {
        for (int k = lane; k < nnz; k += 64) {
            const double a = vals[k]; const int r = T.rowidx[k], c = T.colidx[k];
            if (c < n) A[r * LD + c] = -a;
            else if constexpr (REF) Rp[r] = a;
        }
    };
    // P dense through its own structure (k_fwd_wave_qp's convention: a one-triangle entry fills both slots, a full-structure entry its own)
    auto load_P = [&]() {
        for (int k = lane; k < nnz_p; k += 64) {
            const double a = pvals[k]; const int r = Q.prow[k], c = Q.pcol[k];
            Pm[r * LD + c] = a;
            if (Q.p_tri && r != c) Pm[c * LD + r] = a;
        }
    };
    // REF: y^ = Pi(w) onto the dual cone, row by lane (the decision of the classification pass below)
    auto project = [&](double w) {
        double yh = (lane < z || w > 0) ? w : 0.0;
        if (!ym) yh = 0.0;
        for_cones([&](int r0, int r1) {
            const bool in = lane >= r0 && lane < r1, tail = lane > r0 && lane < r1;
            const double t0 = lane_bcast(w, r0);
            const double nz = sqrt(wave_sum(tail ? w * w : 0.0));
            double lam = 0.0; bool bd = false;
            if (r1 - r0 == 1) lam = t0 >= 0 ? 1.0 : 0.0;
            else if (nz <= t0) lam = 1.0; else if (nz <= -t0) lam = 0.0; else { lam = (t0 + nz) / (2 * nz); bd = true; }
            if (in) yh = (lane == r0) ? (bd ? lam * nz : lam * t0) : lam * w;
        });
        return yh;
    };
    // REF: the KKT residual at (xs, yh, s^ = yh - ws) on the A, P and b in LDS (P as loaded: untransformed at both evaluations); F_x = P x + A^T y^ + c in the
    // variable lanes, F_y in the row lanes; returns rho (a non-finite entry counts as infinite).  Ends behind a wv_sync: the staging vectors, A and P may be rewritten.
    auto kkt_residual = [&](double xs, double yh, double ws, double &Fx, double &Fy) {
        const double inf = __builtin_inf();
        stage_x(xb, xs); stage_y(yb, yh);
        wv_sync();
        const double ax = wv_mv_cols<NX>(A, m, yb, lane) + wv_mv_cols<NX>(Pm, n, xb, lane), ay = wv_mv_rows<NX, MY>(A, m, n, xb, lane);
        double cj = 0.0, bi = 0.0;
        if constexpr (REF) { if (xm) cj = W.q[lane * W.sqk + (long)inst * W.sqb]; }
        if (ym) bi = Rp[lane];
        Fx = xm ? ax + cj : 0.0; Fy = ym ? ay + (yh - ws) - bi : 0.0;
        const double fa = fabs(Fx), fb = fabs(Fy);
        const double mx = wv_max(fmax(fa < inf ? fa : inf, fb < inf ? fb : inf)), sc = wv_max(fmax(fabs(cj), fabs(bi)));
        wv_sync();
        return mx / (1.0 + sc);
    };

    // ---------------------------------------------------------------- prologue: g_x (lane j), g_y (lane i), and A and P in LDS
    clear_all();
    double v = 0.0, gx = 0.0, gy = 0.0, xv = 0.0;
    if constexpr (REF) {
        if (ym) v = W.y[inst * m + lane] - W.s[inst * m + lane];
        if (xm) xv = W.x[inst * n + lane];
        wv_sync();
        load_A(); load_P();
        const double yh = project(v);
        double Fx, Fy;
        rho0 = uniform_d(kkt_residual(xv, yh, v, Fx, Fy));
        if (W.first) rho_cur = rho0;
        gx = Fx; gy = -Fy;
        if (ym) Rp[lane] = 0.0;      // (b has been read: the R buffer is all zeros again, as the elimination expects it)
    } else {
        double yv = 0.0;
        if (ym) { yv = yg[inst * m + lane]; v = yv - sg[inst * m + lane]; }
        if (xm) xv = xg[inst * n + lane];
        if (xm && W.tq) gx = W.tq[lane * W.stqk + (long)inst * W.stqb];
        wv_sync();
        if (W.tA || Q.tP) {      // the tangent's rows, each read once: dA = -tA_eval dense where A goes afterwards, db = +tA_eval[b entries] in the R buffer, tP where P goes
            if (W.tA) {
                const double *tA = W.tA + inst * nnz;
                for (int k = lane; k < nnz; k += 64) {
                    const double a = tA[k]; const int r = T.rowidx[k], c = T.colidx[k];
                    if (c < n) A[r * LD + c] = a; else Rp[r] = a;
                }
            }
            if (Q.tP) {          // entry (r, c) into slot [c][r]: wv_mv_cols below is then row r of tP against x
                const double *tP = Q.tP + inst * (size_t)nnz_p;
                for (int k = lane; k < nnz_p; k += 64) {
                    const double a = tP[k]; const int r = Q.prow[k], c = Q.pcol[k];
                    Pm[c * LD + r] = a;
                    if (Q.p_tri && r != c) Pm[r * LD + c] = a;
                }
            }
            stage_x(xb, xv); stage_y(yb, yv);
            wv_sync();
            const double ax = wv_mv_cols<NX>(A, m, yb, lane), ay = wv_mv_rows<NX, MY>(A, m, n, xb, lane), px = wv_mv_cols<NX>(Pm, n, xb, lane);
            if (xm) gx = (gx - ax) + px;
            if (ym) gy = Rp[lane] + ay;
            wv_sync();
            clear_all();
            wv_sync();
        }
        load_A(); load_P();
    }

    // ---------------------------------------------------------------- classify; per boundary cone gamma_y, gamma_s and the weights u of f + g_x = A^T u
    int rk = RK_FREE;
    bool trow = false;                               // the t-row of a boundary cone
    double u = 0.0, wgt = 0.0;                       // weight of the row in H: theta (z-rows of a boundary cone), -theta (its t-row slot: a_z), else 0
    double c_lam = 0.0, c_inz = 0.0, c_gy = 0.0, c_gs = 0.0;      // of the boundary cone this row belongs to
    if (lane < zl) rk = (lane < z || v > 0) ? RK_EQ : RK_FREE;
    for_cones([&](int r0, int r1) {
        const bool in = lane >= r0 && lane < r1, tail = lane > r0 && lane < r1;
        const double t0 = lane_bcast(v, r0), h0 = lane_bcast(gy, r0);
        const double nz = sqrt(wave_sum(tail ? v * v : 0.0)), zh = wave_sum(tail ? v * gy : 0.0);
        int kind;
        if (r1 - r0 == 1) kind = t0 >= 0 ? 0 : 1;
        else if (nz <= t0) kind = 0; else if (nz <= -t0) kind = 1; else kind = 2;
        if (kind == 0) { if (in) rk = RK_EQ; }
        else if (kind == 1) { if (in) rk = RK_FREE; }
        else {
            const double lam = (t0 + nz) / (2 * nz), th = lam / (1 - lam), inz = 1.0 / nz, zeta = zh / nz;
            if (tail) { u = th * (gy - v * inz * zeta); wgt = th; }
            if (lane == r0) { wgt = -th; trow = true; }
            if (in) { rk = RK_SOCB; c_lam = lam; c_inz = inz; c_gy = (h0 + zeta) * M_SQRT1_2; c_gs = (h0 - zeta) * M_SQRT1_2; }
        }
    });

    // ---------------------------------------------------------------- numbering of the equality rows: the rows in order, then one e_y row per boundary cone
    const bool isEq = ym && rk == RK_EQ;
    const unsigned long long balE = __ballot(isEq), balT = __ballot(trow);
    const int base = __popcll(balE), neq = base + __popcll(balT);
    const int eqi = isEq ? __popcll(balE & lt) : (trow ? base + __popcll(balT & lt) : -1);
    if (neq > n) {      // more active rows than variables: rank deficient by counting (before any store to x, y, s); status 4 as k_backward_ns<FWD, QP>: no list, no re-solve
        if constexpr (REF) {
            if (lane == 0) { W.rstatus[inst] = rst0 | 4; if (W.first) W.resid[2 * inst] = rho0; W.resid[2 * inst + 1] = rho_cur; }
        } else {
            if (xm) W.dx[inst * n + lane] = 0.0;
            if (ym) { W.dy[inst * m + lane] = 0.0; if (W.ds) W.ds[inst * m + lane] = 0.0; }
            if (lane == 0) { if (W.iters) W.iters[inst] = 0; if (adj_status) adj_status[inst] = 4; }
        }
        return;
    }
    wv_sync();      // (the scatters of A and P)

    // ---------------------------------------------------------------- f = -g_x + A^T u (the z-rows of the boundary cones)
    stage_y(yb, u); stage_y(yb2, v);
    if (eqi >= 0) erow[eqi] = lane;
    wv_sync();
    double fx;
    { const double a = wv_mv_cols<NX>(A, m, yb, lane); fx = xm ? a - gx : 0.0; }
    wv_sync();      // (the t-rows are rewritten below)
    // a_z = A_z^T z-hat per boundary cone -> row b of R's buffer for now; e_y's row a_y = (a_0 + a_z) / sqrt 2 over the cone's t-row
    {
        int b = 0;
        for_cones([&](int r0, int r1) {
            if (lane_bcast_i(rk, r0) != RK_SOCB) return;
            if (lane < NX) {
                double az = 0.0;
                for (int i = r0 + 1; i < r1; i++) az = fma(A[i * LD + lane], yb2[i], az);
                az *= lane_bcast(c_inz, r0);
                A[r0 * LD + lane] = (A[r0 * LD + lane] + az) * M_SQRT1_2;
                Rp[b * LD + lane] = az;
            }
            b++;
        });
    }
    wv_sync();

    // ---------------------------------------------------------------- 1. [B | gamma_B] in registers: lane = column, lane n = the right-hand side, row e = c1[e]
    double c1[NX];
    double rtl = 0.0;                              // lane e: rank tolerance of equality row e (CE_RANK_TOL x its largest entry as loaded)
    {
        const int erl = lane < neq ? erow[lane] : 0;
        const double dbv = trow ? c_gy : gy;      // right-hand side of the row's equality
        static_for<NX>([&](auto ec) {
            constexpr int e = decltype(ec)::value;
            c1[e] = 0.0;
            if (e < neq) {
                const int r = lane_bcast_i(erl, e);
                const double a = xm ? A[r * LD + lane] : 0.0, rhs = lane_bcast(dbv, r);
                c1[e] = lane == n ? rhs : a;
                const double rmax = wv_max(fabs(a));
                if (lane == e) rtl = CE_RANK_TOL * (rmax > 0 ? rmax : 1.0);
            }
        });
    }
    // the t-row slots take a_z back (the same lane read a_y from there above): from here on every row of a boundary cone is a weighted row of H
    {
        int b = 0;
        for_cones([&](int r0, int r1) {
            (void)r1;
            if (lane_bcast_i(rk, r0) != RK_SOCB) return;
            if (lane < NX) A[r0 * LD + lane] = Rp[b * LD + lane];
            b++;
        });
    }
    // row elimination with column pivoting.  Per pivot: a DPP max-butterfly on |value| keys with the column in the low mantissa bits, one reciprocal, and per row two
    // v_readlane and one FMA; the scaled pivot row carries 1 + 1/p in the pivot column, so that the pivot columns end as B_1^-1.
    bool cfr = true;                               // lane j: column j is still free
    int pcl = -1, peq = -1, flags = 0;             // lane e: pivot column of equality e ; lane j: equality whose pivot column is j
    static_for<NX>([&](auto ec) {
        constexpr int e = decltype(ec)::value;
        if (e < neq) {
            const double rv = c1[e];
            const double key = __hiloint2double(__double2hiint(rv) & 0x7fffffff, (__double2loint(rv) & ~0xFF) | (255 - lane));
            const double best = wave_reduce_dpp<true>((xm && cfr) ? key : 0.0);
            const int jb = 255 - (__double2loint(best) & 0xFF);
            if (best >= lane_bcast(rtl, e) && jb < n) {
                const double inv = bw_recip(lane_bcast(rv, jb));
                const bool isj = lane == jb;
                const double re = isj ? 1.0 + inv : rv * inv;
                static_for<NG>([&](auto gc) {
                    constexpr int g = decltype(gc)::value;
                    if (8 * g < neq) {          // (uniform; rows past neq hold zeros)
                        double ml[8];
                        static_for<8>([&](auto kc) { constexpr int k = decltype(kc)::value; ml[k] = lane_bcast(c1[8 * g + k], jb); });
                        static_for<8>([&](auto kc) { constexpr int k = decltype(kc)::value; if constexpr (8 * g + k != e) c1[8 * g + k] = fma(-ml[k], re, c1[8 * g + k]); });
                    }
                });
                c1[e] = isj ? inv : re;
                cfr = cfr && !isj;
                if (lane == e) pcl = jb;
                if (isj) peq = e;
            } else { c1[e] = 0.0; flags |= 4; }      // redundant equality row: dropped (eta_e = 0), the instance is flagged
        }
    });
    const bool fr = xm && cfr;
    const unsigned fmask = (unsigned)__ballot(fr);
    // R (free columns), B_1^-1 (pivot columns) and gamma~ (column NX) parked in LDS for x_piv and mu
    static_for<NX>([&](auto ec) {
        constexpr int e = decltype(ec)::value;
        if (e < neq && lane <= n) Rp[e * LD + (xm ? lane : NX)] = c1[e];
    });

    // ---------------------------------------------------------------- 2. null-space transform, lane = column, against the register rows:
    //      a~[j] = a[j] - sum_e a[p_e] R[e][j] (free j);  lane n ends with -t = -sum_e a[p_e] gamma~_e.  The pivot entries of a row stay as loaded.
    const int pcs = pcl >= 0 ? pcl : 0;
    auto transform = [&](double a0) {
        double acc = a0;
        const double apv = __shfl(a0, pcs);
        static_for<NG>([&](auto gc) {
            constexpr int g = decltype(gc)::value;
            if (8 * g < neq) {
                double ap[8];
                static_for<8>([&](auto kc) { constexpr int k = decltype(kc)::value; ap[k] = lane_bcast(apv, 8 * g + k); });
                static_for<8>([&](auto kc) { constexpr int k = decltype(kc)::value; acc = fma(-ap[k], c1[8 * g + k], acc); });
            }
        });
        return acc;
    };
    const unsigned long long wrows = __ballot(wgt != 0.0);
    const int ccol = xm ? lane : NX;      // this lane's column of a weighted row: its own, or the right-hand-side column (lane n)
    for (unsigned long long wm = wrows; wm; wm &= wm - 1) {
        const int i = __builtin_ctzll(wm);
        const double an = transform(xm ? A[i * LD + lane] : 0.0);
        if (fr || lane == n) A[i * LD + ccol] = an;
    }
    { const double ft = transform(fx); if (fr) fx = ft; }      // Z^T f in the free lanes, f itself in the pivot lanes
    // P, first side: every row goes through the transform like a weighted row, W = P Z in the free columns (the pivot columns keep P: step 5 reads them)
    for (int i = 0; i < n; i++) {
        const double pn = transform(xm ? Pm[i * LD + lane] : 0.0);
        if (fr) Pm[i * LD + lane] = pn;
    }
    wv_sync();
    // second side, by symmetry: column b of W read with lane = row (the odd stride LD makes the read conflict-free) through the SAME transform is column b of
    // Z^T P Z, which is also its row b with lane = column; lane n ends with -sum_e W[p_e][b] gamma~_e = -(Z^T P x_p)_b, the right-hand side of that row, on its own.
    // In place: the free rows of column b, and column NX of row b.  No later column reads either slot, and c1[] and G[] are never live together.
    for (unsigned fm = fmask; fm; fm &= fm - 1) {
        const int b = __builtin_ctz(fm);
        const double zn = transform(xm ? Pm[lane * LD + b] : 0.0);
        if (fr) Pm[lane * LD + b] = zn;
        if (lane == n) Pm[b * LD + NX] = zn;
    }
    wv_sync();

    // ---------------------------------------------------------------- 3. reduced Hessian in registers: G[a] (lane b) = (Z^T P Z)[a][b] + sum_k w_k a~_k[a] a~_k[b],
    //      lane n: the right-hand side Z^T f - (Z^T P x_p) - sum_k w_k t_k a~_k.  Pivot rows and columns stay zero.  (Register rows a >= n of a group of eight: as
    //      k_bwd_wave, harmless.)
    double G[NX];
    static_for<NX>([&](auto ac) {      // row a of Z^T P Z with -(Z^T P x_p)_a in lane n; a pivot row, or one past n, starts (and stays) zero
        constexpr int a = decltype(ac)::value;
        G[a] = (((fmask >> a) & 1u) && (fr || lane == n)) ? Pm[a * LD + ccol] : 0.0;
    });
    for (unsigned long long wm = wrows; wm; wm &= wm - 1) {
        const int i = __builtin_ctzll(wm);
        const double av = (fr || lane == n) ? A[i * LD + ccol] : 0.0;
        const double aw = av * lane_bcast(wgt, i);
        static_for<NG>([&](auto gc) {
            constexpr int g = decltype(gc)::value;
            if (8 * g < n) {
                double ml[8];
                static_for<8>([&](auto kc) { constexpr int k = decltype(kc)::value; ml[k] = lane_bcast(aw, 8 * g + k); });
                static_for<8>([&](auto kc) { constexpr int k = decltype(kc)::value; G[8 * g + k] = fma(ml[k], av, G[8 * g + k]); });
            }
        });
    }
    double dg = 0.0;      // lane a: the original diagonal entry of row a (Z^T (H + P) Z's)
    static_for<NX>([&](auto ac) {
        constexpr int a = decltype(ac)::value;
        if (lane == a) dg = G[a];
        const double fa = lane_bcast(fx, a);
        if (lane == n) G[a] += fa;
    });
    // ---------------------------------------------------------------- 4. search-free sweep (Gauss-Jordan on the free columns): the right-hand side ends as x_free
    static_for<NX>([&](auto kc0) {
        constexpr int k = decltype(kc0)::value;
        if (k < n && ((fmask >> k) & 1u)) {          // (uniform)
            const double pv = lane_bcast(G[k], k);
            const bool ok = pv > CE_RANK_TOL * lane_bcast(dg, k);
            const double pinv = ok ? bw_recip(ok ? pv : 1.0) : 0.0;
            if (!ok) flags |= 4;                     // the variable is dropped
            const double rowk = G[k] * pinv;
            static_for<NG>([&](auto gc) {
                constexpr int g = decltype(gc)::value;
                if (8 * g < n) {
                    double ml[8];
                    static_for<8>([&](auto kc) { constexpr int q = decltype(kc)::value; ml[q] = lane_bcast(G[8 * g + q], k); });
                    static_for<8>([&](auto kc) { constexpr int q = decltype(kc)::value; if constexpr (8 * g + q != k) G[8 * g + q] = fma(-ml[q], rowk, G[8 * g + q]); });
                }
            });
            G[k] = rowk;
        }
    });
    double rx = 0.0;
    static_for<NX>([&](auto ac) {
        constexpr int a = decltype(ac)::value;
        const double xa = lane_bcast(G[a], n);
        if (lane == a && fr) rx = xa;
    });

    // ---------------------------------------------------------------- 5. x_piv = gamma~ - R x_free;  q_k = a_k . d_x = t_k + a~_k . x_free for the weighted rows
    stage_x(xb, rx);      // (zeros in the pivot entries)
    wv_sync();
    double qv = wv_mv_rows<NX, MY>(A, m, n, xb, lane);
    const double rdot = wv_mv_rows<NX, MY>(Rp, neq, n, xb, lane);
    const bool zrow = ym && wgt > 0.0;
    qv = zrow ? qv - A[lane * LD + NX] : 0.0;
    const bool prow = lane < neq && pcl >= 0;
    const double xpv = prow ? Rp[lane * LD + NX] - rdot : 0.0;
    wv_sync();
    if (prow) xb[pcl] = xpv;
    stage_x(xb2, 0.0);
    wv_sync();
    rx = xm ? xb[lane] : 0.0;
    // the eliminated rows (lambda = 0) kept their rows of A untouched: a . d_x with the whole of d_x
    const double qfull = wv_mv_rows<NX, MY>(A, m, n, xb, lane);
    // per boundary cone: a_z . d_x = z-hat . (A_z d_x);  q'_i = q_i - z-hat_i (a_z . d_x), so that H d_x = sum over the z-rows of theta a_i q'_i needs no a_z
    double c_zq = 0.0, qp = 0.0;
    for_cones([&](int r0, int r1) {
        if (lane_bcast_i(rk, r0) != RK_SOCB) return;
        const bool in = lane >= r0 && lane < r1, tail = lane > r0 && lane < r1;
        const double zq = wave_sum(tail ? v * qv : 0.0) * lane_bcast(c_inz, r0);
        if (in) c_zq = zq;
        if (tail) qp = qv - v * c_inz * zq;
    });
    // g = ((H + P) d_x - f)[piv] by equality, mu = B_1^-T g.  (P d_x)[p_e]: the pivot columns of the P buffer are as loaded and P is symmetric
    stage_y(yb, zrow ? wgt * qp : 0.0);
    wv_sync();
    const double hq = wv_mv_cols<NX>(A, m, yb, lane) + wv_mv_cols<NX>(Pm, n, xb, lane);
    if (xm && peq >= 0) xb2[peq] = hq - fx;
    wv_sync();
    const double muc = wv_mv_cols<NX>(Rp, neq, xb2, lane);      // lane p_e: mu_e = sum_i B_1^-1[i][e] g_i  (g of a dropped row is 0)
    wv_sync();
    if (xm && peq >= 0) xb2[peq] = muc;
    wv_sync();
    const double mue = eqi >= 0 ? xb2[eqi] : 0.0;               // (a dropped row kept its 0)

    // ---------------------------------------------------------------- epilogue: eta per row (eta_B = -mu), rotated back: dy = W lambda eta, ds = -W (1 - lambda) eta
    double dyv = 0.0, dsv = 0.0;
    if (ym) {
        if (rk == RK_EQ) dyv = -mue;                 // equality rows: their multiplier
        else if (rk == RK_FREE) dsv = gy - qfull;    // eliminated rows: eta = a . d_x - gamma
    }
    for_cones([&](int r0, int r1) {
        if (lane_bcast_i(rk, r0) != RK_SOCB) return;
        const bool tail = lane > r0 && lane < r1;
        const double lam = lane_bcast(c_lam, r0), gyc = lane_bcast(c_gy, r0), gsc = lane_bcast(c_gs, r0), zq = lane_bcast(c_zq, r0), etay = -lane_bcast(mue, r0);
        const int ce = lane_bcast_i(eqi, r0);
        const double ayd = lane_bcast_i(pcl, ce) >= 0 ? gyc : 0.0;      // a_y . d_x = gamma_y (the equality; a dropped row is flagged anyway)
        const double th = lam / (1 - lam), zeta = (gyc - gsc) * M_SQRT1_2;
        const double q0 = M_SQRT2 * ayd - zq;                            // a_0 . d_x
        const double etas = (q0 - zq) * M_SQRT1_2 - gsc;                 // a_s . d_x - gamma_s
        if (tail) {
            const double zh = v * c_inz, pp = (qv - zh * zq) - (gy - zh * zeta);      // (1 - lambda) eta_perp
            dyv = fma(th, pp, zh * etay * M_SQRT1_2); dsv = zh * etas * M_SQRT1_2 - pp;
        }
        if (lane == r0) { dyv = etay * M_SQRT1_2; dsv = -etas * M_SQRT1_2; }
    });

    if constexpr (REF) {
        // ---- x+ = x + dx, v+ = v + (dy - ds), y+ = Pi(v+), s+ = y+ - v+; rho+ on the value row AND the P row scattered again (the elimination transformed
        //      both in place); keep or reject; the record
        const bool flagged = (flags & 4) != 0;
        bool ok = false;
        double rho1 = rho_cur;
        if (!flagged) {          // (uniform)
            const double xn = rx + xv, vn = v + (dyv - dsv);
            wv_sync();
            clear_all();
            wv_sync();
            load_A(); load_P();
            const double yh = project(vn);
            double Fx, Fy;
            rho1 = kkt_residual(xn, yh, vn, Fx, Fy);
            ok = rho1 < fmin(rho0, rho_cur);
            if (ok) {
                if (xm) W.x[inst * n + lane] = xn;
                if (ym) { W.y[inst * m + lane] = yh; W.s[inst * m + lane] = yh - vn; }
            }
        }
        if (lane == 0) {
            W.rstatus[inst] = rst0 | (ok ? 1 : (flagged ? 4 : 2));
            if (ok) W.steps[inst] += 1;
            if (W.first) W.resid[2 * inst] = rho0;
            W.resid[2 * inst + 1] = ok ? rho1 : rho_cur;
        }
    } else {
        if (xm) W.dx[inst * n + lane] = rx;
        if (ym) { W.dy[inst * m + lane] = dyv; if (W.ds) W.ds[inst * m + lane] = dsv; }
        if (lane == 0) {
            if (adj_status) adj_status[inst] = flags;      // (bit 4: a dropped row or variable; the dropped-variable answer stands -- no LSQR has a P term)
            if (W.iters) W.iters[inst] = 0;
        }
    }
}

// ce_jvp_wave_many.h -- k_jvp_wave_many: K tangents through the forward derivative of a SMALL template, one wave per (instance, chunk of at most KC tangents)
// (opt-in: ce_jvp_many_wave).
//
// The system, the rules and the flags are k_newton_wave's forward block (ce_newton_wave.h; read that header first): H d_x + B^T eta_B = f, B d_x = gamma_B by
// null-space elimination, H and B from (A, v = y - s) alone.  There lane = column, lane n carries the one right-hand side through the row elimination, the
// null-space transform, the Gram accumulation and the sweep, and lanes n + 1 .. 63 ride along holding zeros.  Here lane n + k, k < KC, is the right-hand side of
// the chunk's tangent k -- the placement of k_bwd_wave_many (ce_backward_wave_many.h), whose forward twin this kernel is: the four matrix stages are the same
// statements and serve up to KC tangents in the issue cycles of one.
//
// Work split: grid = B x ceil(K / KC), one 64-thread workgroup each, no s_barrier (wv_sync() alone).  The matrix work depends on (A, x, y, s) only and every
// chunk's wave repeats it: a K-tangent call pays ceil(K / KC) factorisations instead of K, in one pass with no stored inverse.
//
// What is decided once per wave, from lanes < n and v alone (so the decisions depend neither on K nor on the chunk): the classification of the rows, the numbering
// of the equalities, the count-out neq > n (status 2), the pivot search, the multipliers and both CE_RANK_TOL tests (status bit 4).  A right-hand-side lane only
// ever receives: the same FMA chain whichever lane and chunk it is, which is why a tangent's result does not depend on its position.
//
// The forward direction's own part, per tangent:
//   in front   g_x,k = tq_k - tA_k^T y and g_y,k = tb_k + tA_k x BEFORE A is loaded, with k_newton_wave's prologue: the tangent's value row is read once, coalesced,
//              and scattered dense through rowidx / colidx into the buffer A takes afterwards (its b entries into the idle R buffer), two one-wave products.  Every
//              tangent's scatter overwrites the same structural positions, so the buffer is cleared once before the first tangent and once behind the last, not K
//              times.  Then per boundary cone gamma_y,k (-> the cone's t-row slot of panel T) and the weights u_k = theta (g - z-hat (z-hat . g_z)) of its z-rows
//              (-> their rows of panel T); behind the load of A, f_k = A^T u_k - g_x,k (one wv_mv_cols per tangent) over g_x,k in panel FX.
//   behind     k_newton_wave's stage 5 and epilogue against column k of the panels: x_piv = gamma~ - R x_free; q = t + a~ . x_free on the weighted rows;
//              mu = B_1^-T (H d_x - f)[piv], eta_B = -mu; eta = a . d_x - gamma on the eliminated rows by one wv_mv_rows over their untouched rows; a_0 . d_x =
//              sqrt 2 gamma_y - a_z . d_x; dx, dy = W lambda eta, ds = -W (1 - lambda) eta.  gamma_y and gamma_s are recomputed from column k of GY (two reductions per
//              boundary cone) instead of kept in two more panels.
// Placement:
//   * registers: c1[NX] (the equality rows [B | gamma_B,0 .. gamma_B,kc-1]), then G[NX] (the reduced Hessian [Z^T H Z | right-hand sides]), never live together.
//   * per-tangent vectors live in the wave's LDS as panels of KC | 1 columns: row i, column k.  A lane = row walk reads (i KP + k) over i -- stride KP, odd --, a
//     lane = right-hand-side walk reads it over k -- stride 1 --: both conflict-free, and the move between the two views is the write in one and the read in the
//     other.  Panels: GY, T, FX, DT (ce_lds_jvp_wave_many.h).
// Outputs per tangent: dx [K][B][n], dy, ds [K][B][m], status and lsqr_iters = 0 [K][B]; bits 2 / 4 are the matrix's, equal across an instance's chunks: the wave
// of chunk 0 alone appends to the re-solve list (the LSQR launch behind this kernel re-solves all K tangents of a listed instance: cone_engine.hip ce_jvp_many_wave).
// LDS is written and read by the owning wave only.  Every loop is bounded by n, m, neq, kc, nnz_aug, the number of cones or a compile-time count.
#pragma once
#include "ce_common.h"
#include "ce_wave_helpers.h"
#include "ce_forward_wave.h"          // wv_sync, lane_bcast, wv_max, wv_mv_cols, wv_mv_rows
#include "ce_backward_wave.h"         // lane_bcast_i, bw_recip
#include "ce_lds_jvp_wave_many.h"     // jvp_wave_many_lds_doubles: the total of the carve below

template <int NX, int MY, int KC, int WPS>
__global__ void __launch_bounds__(64, WPS)
k_jvp_wave_many(DevT T, const double *__restrict__ Avals, const double *__restrict__ xg, const double *__restrict__ yg, const double *__restrict__ sg,
                int *__restrict__ adj_status, int *__restrict__ fix, NsJvpMany W) {
    static_assert(NX <= 32 && MY <= 64 && 64 % NX == 0 && 64 % MY == 0 && NX >= 8 && NX < MY, "k_jvp_wave_many: one lane per row, one per column");
    static_assert(KC >= 1 && KC <= 64 - NX, "k_jvp_wave_many: the right-hand sides ride in the lanes behind the columns");
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int LD = NX + 1, NG = NX / 8, KP = KC | 1;
    const int lane = threadIdx.x;
    const size_t inst = blockIdx.x;
    const int kfirst = (int)blockIdx.y * KC, kc = min(KC, W.K - kfirst);      // this wave's tangents: kfirst .. kfirst + kc
    const int n = T.n, m = T.m, z = T.z, zl = T.z + T.l, nq = T.nq, nnz = T.nnz_aug;
    double *A = sm, *Rp = A + m * LD, *xb = Rp + NX * LD, *xb2 = xb + NX, *yb = xb2 + NX, *yb2 = yb + MY;
    int *erow = (int *)(yb2 + MY);
    double *Gy = yb2 + MY + (NX + 1) / 2, *Tp = Gy + m * KP, *FX = Tp + m * KP, *Dt = FX + NX * KP;
    const bool xm = lane < n, ym = lane < m;
    const int rl = lane - n;                      // the tangent of the chunk this lane is the right-hand side of
    const bool isr = rl >= 0 && rl < kc;
    const unsigned long long lt = (1ull << lane) - 1ull;

    int qe = 0;      // first row behind the second-order cone this lane's row belongs to (k_fwd_wave's walk)
    if (ym && lane >= zl) qe = T.qoff[T.rowcone[lane] + 1];
    auto for_cones = [&](auto &&f) {
        int r0 = zl;
        for (int c = 0; c < nq; c++) { const int r1 = __builtin_amdgcn_readlane(qe, r0); f(r0, r1); r0 = r1; }
    };
    auto stage_x = [&](double *buf, double v) { if (lane < NX) buf[lane] = v; };
    auto stage_y = [&](double *buf, double v) { if (lane < MY) buf[lane] = v; };
    auto clear_A = [&]() { for (int i = lane; i < (m + NX) * LD; i += 64) A[i] = 0.0; };      // (A and R are contiguous)

    const double yv = ym ? yg[inst * m + lane] : 0.0;
    const double v = ym ? yv - sg[inst * m + lane] : 0.0;

    // ---------------------------------------------------------------- classify (k_newton_wave's rules; what depends on v alone)
    int rk = RK_FREE;
    bool trow = false;                               // the t-row of a boundary cone
    double wgt = 0.0;                                // weight of the row in H: theta (z-rows of a boundary cone), -theta (its t-row slot: a_z), else 0
    double c_lam = 0.0, c_inz = 0.0, c_nz = 0.0;     // of the boundary cone this row belongs to
    if (lane < zl) rk = (lane < z || v > 0) ? RK_EQ : RK_FREE;
    for_cones([&](int r0, int r1) {
        const bool in = lane >= r0 && lane < r1, tail = lane > r0 && lane < r1;
        const double t0 = lane_bcast(v, r0);
        const double nz = sqrt(wave_sum(tail ? v * v : 0.0));
        int kind;
        if (r1 - r0 == 1) kind = t0 >= 0 ? 0 : 1;
        else if (nz <= t0) kind = 0; else if (nz <= -t0) kind = 1; else kind = 2;
        if (kind == 0) { if (in) rk = RK_EQ; }
        else if (kind == 1) { if (in) rk = RK_FREE; }
        else {
            const double lam = (t0 + nz) / (2 * nz), th = lam / (1 - lam);
            if (tail) wgt = th;
            if (lane == r0) { wgt = -th; trow = true; }
            if (in) { rk = RK_SOCB; c_lam = lam; c_inz = 1.0 / nz; c_nz = nz; }
        }
    });

    // ---------------------------------------------------------------- numbering of the equality rows: the rows in order, then one e_y row per boundary cone
    const bool isEq = ym && rk == RK_EQ;
    const unsigned long long balE = __ballot(isEq), balT = __ballot(trow);
    const int base = __popcll(balE), neq = base + __popcll(balT);
    const int eqi = isEq ? __popcll(balE & lt) : (trow ? base + __popcll(balT & lt) : -1);
    if (neq > n) {      // more active rows than variables: rank deficient by counting (zero outputs, flagged for every k, listed once)
        for (int k = 0; k < kc; k++) {
            const long kk = kfirst + k;
            if (xm) W.dx[kk * W.sxk + (long)inst * n + lane] = 0.0;
            if (ym) { W.dy[kk * W.syk + (long)inst * m + lane] = 0.0; if (W.ds) W.ds[kk * W.syk + (long)inst * m + lane] = 0.0; }
            if (lane == 0) { if (W.iters) W.iters[kk * W.sak + (long)inst] = 0; if (adj_status) adj_status[kk * W.sak + (long)inst] = 2; }
        }
        if (lane == 0 && fix && blockIdx.y == 0) fix[1 + atomicAdd(fix, 1)] = (int)inst;
        return;
    }

    // ---------------------------------------------------------------- per tangent, before A: g_x,k -> FX[., k], g_y,k -> GY[., k]; of a boundary cone gamma_y,k ->
    //      T[t-row, k] and the weights u_k -> T[z-rows, k] (0 in every other row)
    clear_A();
    stage_x(xb, xm ? xg[inst * n + lane] : 0.0); stage_y(yb, yv);
    for (int k = 0; k < kc; k++) {
        const long kk = kfirst + k;
        double gx = 0.0, gy = 0.0;
        if (xm && W.tq) gx = W.tq[kk * W.stqk + (long)inst * W.stqb + lane];
        if (W.tA) {      // the tangent's value row, read once: dA = -tA_eval dense where A goes afterwards, db = +tA_eval[b entries] in the R buffer
            const double *tA = W.tA + kk * W.stAk + (long)inst * W.stAb;
            wv_sync();      // (the clear and the staging; the products of the tangent before)
            for (int e = lane; e < nnz; e += 64) {
                const double a = tA[e]; const int r = T.rowidx[e], c = T.colidx[e];
                if (c < n) A[r * LD + c] = a; else Rp[r] = a;
            }
            wv_sync();
            const double ax = wv_mv_cols<NX>(A, m, yb, lane), ay = wv_mv_rows<NX, MY>(A, m, n, xb, lane);
            if (xm) gx -= ax;
            if (ym) gy = Rp[lane] + ay;
        }
        double u = 0.0;
        for_cones([&](int r0, int r1) {
            if (lane_bcast_i(rk, r0) != RK_SOCB) return;
            const bool tail = lane > r0 && lane < r1;
            const double h0 = lane_bcast(gy, r0), zeta = wave_sum(tail ? v * gy : 0.0) / lane_bcast(c_nz, r0);
            if (tail) u = wgt * (gy - v * c_inz * zeta);
            if (lane == r0) u = (h0 + zeta) * M_SQRT1_2;      // gamma_y in the t-row's slot (the row's own weight in f is 0)
        });
        if (ym) { Gy[lane * KP + k] = gy; Tp[lane * KP + k] = u; }
        if (xm) FX[lane * KP + k] = gx;
    }
    wv_sync();
    if (W.tA) { clear_A(); wv_sync(); }
    // ---------------------------------------------------------------- load: A = -A_cvx dense through the template's structure
    {
        const double *vals = Avals + inst * nnz;
        for (int e = lane; e < nnz; e += 64) {
            const double a = vals[e]; const int r = T.rowidx[e], c = T.colidx[e];
            if (c < n) A[r * LD + c] = -a;
        }
    }
    if (eqi >= 0) erow[eqi] = lane;
    stage_y(yb2, v);
    // f_k = A^T u_k - g_x,k over g_x,k (the z-rows of the boundary cones; the t-rows still a_0, weight 0)
    for (int k = 0; k < kc; k++) {
        wv_sync();      // (the scatter of A and the panels; the product of the tangent before has read yb)
        stage_y(yb, (ym && !trow) ? Tp[lane * KP + k] : 0.0);
        wv_sync();
        const double a = wv_mv_cols<NX>(A, m, yb, lane);
        if (xm) FX[lane * KP + k] = a - FX[lane * KP + k];
    }
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

    // ---------------------------------------------------------------- 1. [B | gamma_B,0 .. gamma_B,kc-1] in registers: lane = column, lane n + k = right-hand side k, row e = c1[e]
    double c1[NX];
    double rtl = 0.0;                              // lane e: rank tolerance of equality row e (CE_RANK_TOL x its largest entry as loaded)
    {
        const int erl = lane < neq ? erow[lane] : 0;
        static_for<NX>([&](auto ec) {
            constexpr int e = decltype(ec)::value;
            c1[e] = 0.0;
            if (e < neq) {
                const int r = lane_bcast_i(erl, e);
                const double a = xm ? A[r * LD + lane] : 0.0;
                const double rhs = isr ? (((balT >> r) & 1ull) ? Tp[r * KP + rl] : Gy[r * KP + rl]) : 0.0;      // gamma_y,k of a boundary cone, g_y,k of a row
                c1[e] = xm ? a : rhs;
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
    // row elimination with column pivoting (k_newton_wave's, statement by statement; the search reads lanes < n, the update runs over all 64)
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
                        static_for<8>([&](auto kc8) { constexpr int k = decltype(kc8)::value; ml[k] = lane_bcast(c1[8 * g + k], jb); });
                        static_for<8>([&](auto kc8) { constexpr int k = decltype(kc8)::value; if constexpr (8 * g + k != e) c1[8 * g + k] = fma(-ml[k], re, c1[8 * g + k]); });
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
    // R (free columns) and B_1^-1 (pivot columns) parked in LDS for x_piv and mu, gamma~_k in DT[., k]
    static_for<NX>([&](auto ec) {
        constexpr int e = decltype(ec)::value;
        if (e < neq) {
            if (xm) Rp[e * LD + lane] = c1[e];
            else if (isr) Dt[e * KP + rl] = c1[e];
        }
    });

    // ---------------------------------------------------------------- 2. null-space transform, lane = column, against the register rows: a~[j] = a[j] - sum_e a[p_e] R[e][j]
    //      (free j); lane n + k ends with -t_k = -sum_e a[p_e] gamma~_e,k on its own.  The pivot entries of a row stay as loaded.
    const int pcs = pcl >= 0 ? pcl : 0;
    auto transform = [&](double a0) {
        double acc = a0;
        const double apv = __shfl(a0, pcs);
        static_for<NG>([&](auto gc) {
            constexpr int g = decltype(gc)::value;
            if (8 * g < neq) {
                double ap[8];
                static_for<8>([&](auto kc8) { constexpr int k = decltype(kc8)::value; ap[k] = lane_bcast(apv, 8 * g + k); });
                static_for<8>([&](auto kc8) { constexpr int k = decltype(kc8)::value; acc = fma(-ap[k], c1[8 * g + k], acc); });
            }
        });
        return acc;
    };
    const unsigned long long wrows = __ballot(wgt != 0.0);
    for (unsigned long long wm = wrows; wm; wm &= wm - 1) {
        const int i = __builtin_ctzll(wm);
        const double an = transform(xm ? A[i * LD + lane] : 0.0);
        if (fr) A[i * LD + lane] = an;
        else if (isr) Tp[i * KP + rl] = an;      // (over u_k / gamma_y,k in the row's slot: f_k and stage 1 have read them)
    }
    for (int k = 0; k < kc; k++) {      // Z^T f_k in the free rows of FX[., k], f_k itself in the pivot rows
        const double ft = transform(xm ? FX[lane * KP + k] : 0.0);
        if (fr) FX[lane * KP + k] = ft;
    }
    wv_sync();

    // ---------------------------------------------------------------- 3. reduced Hessian in registers: G[a] (lane b) = sum_i w_i a~_i[a] a~_i[b]; lane n + k: the
    //      right-hand side (Z^T f_k)[a] - sum_i w_i t_i,k a~_i[a].  Pivot rows and columns stay zero.  (Register rows a >= n pick up right-hand-side lanes' values
    //      through the groups of eight and are swept along: harmless, as in k_bwd_wave_many -- never pivot rows, and only rows < n are read.)
    double G[NX];
    static_for<NX>([&](auto ac) { G[decltype(ac)::value] = 0.0; });
    for (unsigned long long wm = wrows; wm; wm &= wm - 1) {
        const int i = __builtin_ctzll(wm);
        const double av = fr ? A[i * LD + lane] : (isr ? Tp[i * KP + rl] : 0.0);
        const double aw = av * lane_bcast(wgt, i);
        static_for<NG>([&](auto gc) {
            constexpr int g = decltype(gc)::value;
            if (8 * g < n) {
                double ml[8];
                static_for<8>([&](auto kc8) { constexpr int k = decltype(kc8)::value; ml[k] = lane_bcast(aw, 8 * g + k); });
                static_for<8>([&](auto kc8) { constexpr int k = decltype(kc8)::value; G[8 * g + k] = fma(ml[k], av, G[8 * g + k]); });
            }
        });
    }
    double dg = 0.0;      // lane a: the original diagonal entry of row a
    static_for<NX>([&](auto ac) {
        constexpr int a = decltype(ac)::value;
        if (lane == a) dg = G[a];
        if (a < n && isr) G[a] += FX[a * KP + rl];
    });
    // ---------------------------------------------------------------- 4. search-free sweep (Gauss-Jordan on the free columns): right-hand side k ends as x_free,k
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
                    static_for<8>([&](auto kc8) { constexpr int q = decltype(kc8)::value; ml[q] = lane_bcast(G[8 * g + q], k); });
                    static_for<8>([&](auto kc8) { constexpr int q = decltype(kc8)::value; if constexpr (8 * g + q != k) G[8 * g + q] = fma(-ml[q], rowk, G[8 * g + q]); });
                }
            });
            G[k] = rowk;
        }
    });
    // x_free,k over Z^T f_k in the free rows of FX[., k] (the pivot rows keep f_k, which g = (H d_x - f)[piv] needs)
    static_for<NX>([&](auto ac) {
        constexpr int a = decltype(ac)::value;
        if (a < n && ((fmask >> a) & 1u) && isr) FX[a * KP + rl] = G[a];
    });

    // ---------------------------------------------------------------- 5. per tangent, k_newton_wave's statements against column k of the panels:
    //      x_piv = gamma~ - R x_free;  q = t + a~ . x_free for the weighted rows;  g = (H d_x - f)[piv], mu = B_1^-T g;  eta per row, rotated back;  the outputs
    const bool zrow = ym && wgt > 0.0;
    const bool prow = lane < neq && pcl >= 0;
    for (int k = 0; k < kc; k++) {
        const long kk = kfirst + k;
        wv_sync();      // (the panels behind the sweep; the staging vectors behind the tangent before)
        const double fk = xm ? FX[lane * KP + k] : 0.0;      // free lanes: x_free ; pivot lanes: f
        const double gy = ym ? Gy[lane * KP + k] : 0.0;
        stage_x(xb, fr ? fk : 0.0);      // (zeros in the pivot entries)
        wv_sync();
        double qv = wv_mv_rows<NX, MY>(A, m, n, xb, lane);
        const double rdot = wv_mv_rows<NX, MY>(Rp, neq, n, xb, lane);
        qv = zrow ? qv - Tp[lane * KP + k] : 0.0;
        const double xpv = prow ? Dt[lane * KP + k] - rdot : 0.0;
        wv_sync();
        if (prow) xb[pcl] = xpv;
        stage_x(xb2, 0.0);
        wv_sync();
        const double rx = xm ? xb[lane] : 0.0;
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
        // g = (H d_x - f)[piv] by equality, mu = B_1^-T g
        stage_y(yb, zrow ? wgt * qp : 0.0);
        wv_sync();
        const double hq = wv_mv_cols<NX>(A, m, yb, lane);
        if (xm && peq >= 0) xb2[peq] = hq - fk;
        wv_sync();
        const double muc = wv_mv_cols<NX>(Rp, neq, xb2, lane);      // lane p_e: mu_e = sum_i B_1^-1[i][e] g_i  (g of a dropped row is 0)
        wv_sync();
        if (xm && peq >= 0) xb2[peq] = muc;
        wv_sync();
        const double mue = eqi >= 0 ? xb2[eqi] : 0.0;               // (a dropped row kept its 0)

        // eta per row (eta_B = -mu), rotated back: dy = W lambda eta, ds = -W (1 - lambda) eta
        double dyv = 0.0, dsv = 0.0;
        if (ym) {
            if (rk == RK_EQ) dyv = -mue;                 // equality rows: their multiplier
            else if (rk == RK_FREE) dsv = gy - qfull;    // eliminated rows: eta = a . d_x - gamma
        }
        for_cones([&](int r0, int r1) {
            if (lane_bcast_i(rk, r0) != RK_SOCB) return;
            const bool tail = lane > r0 && lane < r1;
            const double h0 = lane_bcast(gy, r0), zeta = wave_sum(tail ? v * gy : 0.0) / lane_bcast(c_nz, r0);      // (as the first loop computed them from the same g_y)
            const double gyc = (h0 + zeta) * M_SQRT1_2, gsc = (h0 - zeta) * M_SQRT1_2;
            const double lam = lane_bcast(c_lam, r0), zq = lane_bcast(c_zq, r0), etay = -lane_bcast(mue, r0);
            const int ce = lane_bcast_i(eqi, r0);
            const double ayd = lane_bcast_i(pcl, ce) >= 0 ? gyc : 0.0;      // a_y . d_x = gamma_y (the equality; a dropped row is flagged anyway)
            const double th = lam / (1 - lam);
            const double q0 = M_SQRT2 * ayd - zq;                            // a_0 . d_x
            const double etas = (q0 - zq) * M_SQRT1_2 - gsc;                 // a_s . d_x - gamma_s
            if (tail) {
                const double zh = v * c_inz, pp = (qv - zh * zq) - (gy - zh * zeta);      // (1 - lambda) eta_perp
                dyv = fma(th, pp, zh * etay * M_SQRT1_2); dsv = zh * etas * M_SQRT1_2 - pp;
            }
            if (lane == r0) { dyv = etay * M_SQRT1_2; dsv = -etas * M_SQRT1_2; }
        });

        if (xm) W.dx[kk * W.sxk + (long)inst * n + lane] = rx;
        if (ym) { W.dy[kk * W.syk + (long)inst * m + lane] = dyv; if (W.ds) W.ds[kk * W.syk + (long)inst * m + lane] = dsv; }
        if (lane == 0) {
            if (adj_status) adj_status[kk * W.sak + (long)inst] = flags;
            if (W.iters) W.iters[kk * W.sak + (long)inst] = 0;
        }
    }
    if (lane == 0 && fix && (flags & 4) && blockIdx.y == 0) fix[1 + atomicAdd(fix, 1)] = (int)inst;      // listed once: the LSQR launch replaces all K answers
}

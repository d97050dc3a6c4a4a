// ce_backward_wave_many_qp.h -- k_bwd_wave_many_qp: K cotangents through the adjoint of a SMALL template with a QUADRATIC objective inside the kernels, one wave
// per (instance, chunk of at most KC cotangents) (opt-in: ce_vjp_qp_many_wave, ce_vjp_qp_many_params_wave).
//
// The system and the answers are k_backward_ns<..., QP, MANY>'s (ce_backward_ns.h), r_tau pinned to 0; for every cotangent k
//        (H + P) r_x,k - B^T mu_k = f_k,   B r_x,k = d_B,k,       H = sum_c theta_c (A_z^T A_z - a_z a_z^T)  over the boundary cones,   B = the neq equality rows,
// by the null-space elimination of k_bwd_wave (ce_backward_wave.h; read that header first).  Two restatements meet here, RESTATED once more and not shared through
// edits to either header (a restated kernel cannot touch bwd_wave_many.o's or bwd_wave_qp.o's device code -- k_newton_wave's choice):
//   * k_bwd_wave_many's work split and placement (ce_backward_wave_many.h): grid = B x ceil(K / KC), one 64-thread workgroup each, wv_sync() alone; lane j < n is
//     column j, lane n + k, k < KC, the right-hand side of the chunk's cotangent k through the row elimination, the transform, the Gram accumulation and the sweep; the
//     per-cotangent vectors live in four LDS panels of stride KC | 1 (D, T, FX, DT) and the vector stages in front of and behind the matrix stages run per cotangent.
//   * k_bwd_wave_qp's P terms (ce_backward_wave_qp.h): P is a third dense LDS matrix behind A and R | B_1^-1, scattered through the structure's (row, column)
//     arrays (a one-triangle entry fills both slots); while the eliminated rows c1[] are registers every row of P goes through transform() and then every FREE
//     column b of W = P Z, read with lane = row, goes through it again: lanes < n end with row b of Z^T P Z, written back in place.
// What the two make together: in that second pass lane n + k holds d~_k in c1[], starts from 0 and ends with -(Z^T P x_p,k)_b -- the reduced right-hand side's P
// share of EVERY cotangent of the chunk for the one transform the single-cotangent kernel pays.  It is added in place to (Z^T f_k)_b in panel FX (the lane that
// owns column k of the panel; no fifth panel, and column NX of the P buffer is unused here), so stage 3 starts G[a] from row a of the P buffer in lanes < n, from 0
// in the right-hand-side lanes, and adds FX behind the Gram as k_bwd_wave_many does.  c1[] and G[] are never live together.
//   stage 3   dg, the diagonal the sweep's rank test compares against, is Z^T (H + P) Z's.  No weighted row and neq = 0: the reduced Hessian is P alone.
//   stage 5   per cotangent g = ((H + P) r_x,k - f_k)[piv]: (P r_x,k)[p_e] is one more wv_mv_cols over the P buffer with the staged r_x,k -- pivot columns as loaded.
//   outputs   per cotangent the dA row, dq = -r_x and dP[k] = ce_dP_entry(...) through the structure, doubled off the diagonal of a one-triangle structure; in
//             record mode (W.rec: ce_vjp_qp_many_params' layout, rpitch m + 1 + n) r_y, r_tau = 0, r_x and neither dA nor dP.
//   flags     the QP elimination's: neq > n is status 4 with zero outputs for every k; a dropped equality row or variable sets bit 4 and the dropped-variable answer
//             stands.  Bit 8 is never set; no re-solve list, no LSQR (none has a P term).  adj_status is [K][B].
// What is decided once per wave, from lanes < n alone (so neither K nor the chunk enters): the classification, the numbering, the count-out, the pivot search and both
// CE_RANK_TOL tests.  A right-hand-side lane only ever receives the same FMA chain whichever lane and chunk it is: a cotangent's result does not depend on its position.
// LDS is written and read by the owning wave only.  Every loop is bounded by n, m, neq, kc, nnz, nnz_p, the number of cones or a compile-time count.
#pragma once
#include "ce_common.h"
#include "ce_wave_helpers.h"
#include "ce_forward_wave.h"             // wv_sync, lane_bcast, wv_max, wv_mv_cols, wv_mv_rows
#include "ce_backward_wave.h"            // lane_bcast_i, bw_recip
#include "ce_dA_entry.h"                 // ce_dA_entry, ce_dP_entry: shared with k_backward_ns
#include "ce_lds_bwd_wave_many_qp.h"     // bwd_wave_many_qp_lds_doubles: the total of the carve below

template <int NX, int MY, int KC, int WPS>
__global__ void __launch_bounds__(64, WPS)
k_bwd_wave_many_qp(DevT T, const double *__restrict__ Avals, const double *__restrict__ xg, const double *__restrict__ yg, const double *__restrict__ sg,
                   const double *__restrict__ dxg, const double *__restrict__ dyg, double *__restrict__ dAo, double *__restrict__ dqo, long sdqk, long sdqb,
                   int *__restrict__ adj_status, BwdWaveManyQp W) {
    static_assert(NX <= 32 && MY <= 64 && 64 % NX == 0 && 64 % MY == 0 && NX >= 8 && NX < MY, "k_bwd_wave_many_qp: one lane per row, one per column");
    static_assert(KC >= 1 && KC <= 64 - NX, "k_bwd_wave_many_qp: the right-hand sides ride in the lanes behind the columns");
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int LD = NX + 1, NG = NX / 8, KP = KC | 1;
    const int lane = threadIdx.x;
    const size_t inst = blockIdx.x;
    const int kfirst = (int)blockIdx.y * KC, kc = min(KC, W.K - kfirst);      // this wave's cotangents: kfirst .. kfirst + kc
    const int n = T.n, m = T.m, z = T.z, zl = T.z + T.l, nq = T.nq, nnz = T.nnz_aug, nnz_p = W.nnz_p;
    double *A = sm, *Rp = A + m * LD, *Pm = Rp + NX * LD, *xb = Pm + n * LD, *xb2 = xb + NX, *yb = xb2 + NX, *yb2 = yb + MY;
    int *erow = (int *)(yb2 + MY);
    double *Dp = yb2 + MY + (NX + 1) / 2, *Tp = Dp + m * KP, *FX = Tp + m * KP, *Dt = FX + NX * KP;
    const bool xm = lane < n, ym = lane < m;
    const int rl = lane - n;                      // the cotangent of the chunk this lane is the right-hand side of
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

    // ---------------------------------------------------------------- load: A = -A_cvx dense through the template's structure, P dense through its own
    //      (k_fwd_wave_qp's convention: a one-triangle entry fills both slots, a full-structure entry its own)
    for (int i = lane; i < (m + NX + n) * LD; i += 64) A[i] = 0.0;      // (A, R and P are contiguous)
    const double v = ym ? yg[inst * m + lane] - sg[inst * m + lane] : 0.0;
    wv_sync();
    {
        const double *vals = Avals + inst * nnz;
        for (int k = lane; k < nnz; k += 64) {
            const double a = vals[k]; const int r = T.rowidx[k], c = T.colidx[k];
            if (c < n) A[r * LD + c] = -a;
        }
        const double *pv = W.P + inst * (size_t)nnz_p;
        for (int k = lane; k < nnz_p; k += 64) {
            const double a = pv[k]; const int r = W.prow[k], c = W.pcol[k];
            Pm[r * LD + c] = a;
            if (W.p_tri && r != c) Pm[c * LD + r] = a;
        }
    }

    // ---------------------------------------------------------------- classify (k_bwd_wave's rules; what depends on v alone)
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
    if (neq > n) {      // more active rows than variables: rank deficient by counting (zero gradients, status 4 for every k as k_backward_ns<QP>: no list, no re-solve)
        for (int k = 0; k < kc; k++) {
            const long kk = kfirst + k;
            if (W.rec) {
                double *const rec = W.rec + kk * W.srk + (long)inst * W.rpitch;
                for (int i = lane; i < m + 1 + n; i += 64) rec[i] = 0.0;
            } else {
                double *const dArow = dAo + kk * W.sAk + (long)inst * nnz, *const dProw = W.dP + kk * W.sPk + (long)inst * nnz_p;
                for (int i = lane; i < nnz; i += 64) dArow[i] = 0.0;
                for (int i = lane; i < nnz_p; i += 64) dProw[i] = 0.0;
            }
            if (lane <= n) dqo[kk * W.sqk + lane * sdqk + (long)inst * sdqb] = 0.0;
            if (lane == 0 && adj_status) adj_status[kk * W.sak + (long)inst] = 4;
        }
        return;
    }
    if (eqi >= 0) erow[eqi] = lane;
    stage_y(yb2, v);
    wv_sync();      // (the scatters of A and P)

    // ---------------------------------------------------------------- per cotangent: d_k = DPi(v) dy_k -> D[., k], e_y . d_k of a boundary cone -> T[t-row, k] (until the
    //      transform), f_k = dx_k + A^T u_k -> FX[., k]  (all rows of the boundary cones at once, the t-rows still a_0)
    for (int k = 0; k < kc; k++) {
        const long kk = kfirst + k;
        double d = ym ? dyg[kk * W.syk + (long)inst * m + lane] : 0.0;
        const double dxv = xm ? dxg[kk * W.sxk + (long)inst * n + lane] : 0.0;
        double u = 0.0;
        if (lane < zl && rk != RK_EQ) d = 0.0;
        for_cones([&](int r0, int r1) {
            const bool in = lane >= r0 && lane < r1, tail = lane > r0 && lane < r1;
            const int ck = lane_bcast_i(rk, r0);
            if (ck == RK_EQ) return;
            if (ck == RK_FREE) { if (in) d = 0.0; return; }
            const double t0 = lane_bcast(v, r0), h0 = lane_bcast(d, r0), nz = lane_bcast(c_nz, r0), lam = lane_bcast(c_lam, r0), inz = lane_bcast(c_inz, r0);
            const double zh = wave_sum(tail ? v * d : 0.0);
            const double i2n = 1.0 / (2 * nz), cz = t0 * zh / (nz * nz);
            const double di = tail ? (v * h0 + (t0 + nz) * d - v * cz) * i2n : 0.0;
            const double zd = wave_sum(tail ? v * di : 0.0);
            const double d0 = (nz * h0 + zh) * i2n, zdn = zd / nz, eyd = (d0 + zdn) * M_SQRT1_2, esd = (d0 - zdn) * M_SQRT1_2;
            const double il = 1.0 / (1 - lam);
            const double k0c = (esd * (1 - il) - eyd * il) * M_SQRT1_2, kzc = (-esd * (1 - il) - eyd * il) * M_SQRT1_2;
            if (tail) { d = di; u = fma(il, di, v * inz * kzc); }
            if (lane == r0) { d = d0; u = fma(il, d0, k0c); Tp[r0 * KP + k] = eyd; }
        });
        wv_sync();      // (the product of the cotangent before has read yb)
        stage_y(yb, u);
        if (ym) Dp[lane * KP + k] = d;
        wv_sync();
        const double a = wv_mv_cols<NX>(A, m, yb, lane);
        if (xm) FX[lane * KP + k] = dxv + a;
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

    // ---------------------------------------------------------------- 1. [B | d_B,0 .. d_B,kc-1] in registers: lane = column, lane n + k = right-hand side k, row e = c1[e]
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
                const double rhs = isr ? (((balT >> r) & 1ull) ? Tp[r * KP + rl] : Dp[r * KP + rl]) : 0.0;      // e_y . d_k of a boundary cone, d_k of a row
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
    // row elimination with column pivoting (k_bwd_wave's, statement by statement; the search reads lanes < n, the update runs over all 64)
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
            } else { c1[e] = 0.0; flags |= 4; }      // redundant equality row: dropped (mu_e = 0), the instance is flagged
        }
    });
    const bool fr = xm && cfr;
    const unsigned fmask = (unsigned)__ballot(fr);
    // R (free columns) and B_1^-1 (pivot columns) parked in LDS for x_piv and mu, d~_k in DT[., k]
    static_for<NX>([&](auto ec) {
        constexpr int e = decltype(ec)::value;
        if (e < neq) {
            if (xm) Rp[e * LD + lane] = c1[e];
            else if (isr) Dt[e * KP + rl] = c1[e];
        }
    });

    // ---------------------------------------------------------------- 2. null-space transform, lane = column, against the register rows: a~[j] = a[j] - sum_e a[p_e] R[e][j]
    //      (free j); lane n + k ends with -t_k = -sum_e a[p_e] d~_e,k on its own.  The pivot entries of a row stay as loaded.
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
        else if (isr) Tp[i * KP + rl] = an;      // (over e_y . d_k in a t-row's slot: the same lane read it in stage 1)
    }
    for (int k = 0; k < kc; k++) {      // Z^T f_k in the free rows of FX[., k], f_k itself in the pivot rows
        const double ft = transform(xm ? FX[lane * KP + k] : 0.0);
        if (fr) FX[lane * KP + k] = ft;
    }
    // P, first side: every row goes through the transform like a weighted row, W = P Z in the free columns (the pivot columns keep P: stage 5 reads them)
    for (int i = 0; i < n; i++) {
        const double pn = transform(xm ? Pm[i * LD + lane] : 0.0);
        if (fr) Pm[i * LD + lane] = pn;
    }
    wv_sync();
    // second side, by symmetry: column b of W read with lane = row (the odd stride LD makes the read conflict-free) through the SAME transform is column b of
    // Z^T P Z, which is also its row b with lane = column; lane n + k starts from 0 and ends with -sum_e W[p_e][b] d~_e,k = -(Z^T P x_p,k)_b, which joins
    // (Z^T f_k)_b where it lies: row b of FX, the lane's own column.  In place: no later column reads the free rows of column b.
    for (unsigned fm = fmask; fm; fm &= fm - 1) {
        const int b = __builtin_ctz(fm);
        const double zn = transform(xm ? Pm[lane * LD + b] : 0.0);
        if (fr) Pm[lane * LD + b] = zn;
        else if (isr) FX[b * KP + rl] += zn;
    }
    wv_sync();

    // ---------------------------------------------------------------- 3. reduced Hessian in registers: G[a] (lane b) = (Z^T P Z)[a][b] + sum_i w_i a~_i[a] a~_i[b]; lane
    //      n + k: the right-hand side (Z^T f_k - Z^T P x_p,k)[a] - sum_i w_i t_i,k a~_i[a].  Pivot rows and columns stay zero.  (Register rows a >= n pick up
    //      right-hand-side lanes' values through the groups of eight and are swept along: harmless, as in k_bwd_wave -- never pivot rows, and only rows < n are read.)
    double G[NX];
    static_for<NX>([&](auto ac) {      // row a of Z^T P Z; a pivot row, or one past n, starts (and stays) zero
        constexpr int a = decltype(ac)::value;
        G[a] = (((fmask >> a) & 1u) && fr) ? Pm[a * LD + lane] : 0.0;
    });
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
    double dg = 0.0;      // lane a: the original diagonal entry of row a of Z^T (H + P) Z
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
    // x_free,k over the reduced right-hand side in the free rows of FX[., k] (the pivot rows keep f_k, which g = ((H + P) r_x - f)[piv] needs)
    static_for<NX>([&](auto ac) {
        constexpr int a = decltype(ac)::value;
        if (a < n && ((fmask >> a) & 1u) && isr) FX[a * KP + rl] = G[a];
    });

    // ---------------------------------------------------------------- 5. per cotangent, k_bwd_wave_qp's statements against column k of the panels:
    //      x_piv = d~ - R x_free;  q = t + a~ . x_free for the weighted rows;  g = ((H + P) r_x - f)[piv], mu = B_1^-T g;  r_y;  the outputs
    const bool zrow = ym && wgt > 0.0;
    const bool prow = lane < neq && pcl >= 0;
    const double xv = xm ? xg[inst * n + lane] : 0.0, yv = ym ? yg[inst * m + lane] : 0.0;
    for (int k = 0; k < kc; k++) {
        const long kk = kfirst + k;
        wv_sync();      // (the panels behind the sweep; the staging vectors behind the cotangent before)
        const double fk = xm ? FX[lane * KP + k] : 0.0;      // free lanes: x_free ; pivot lanes: f
        const double d = ym ? Dp[lane * KP + k] : 0.0;
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
        // per boundary cone: a_z . r_x = z-hat . (A_z r_x);  q'_i = q_i - z-hat_i (a_z . r_x)
        double c_zq = 0.0, qp = 0.0;
        for_cones([&](int r0, int r1) {
            if (lane_bcast_i(rk, r0) != RK_SOCB) return;
            const bool in = lane >= r0 && lane < r1, tail = lane > r0 && lane < r1;
            const double zq = wave_sum(tail ? v * qv : 0.0) * lane_bcast(c_inz, r0);
            if (in) c_zq = zq;
            if (tail) qp = qv - v * c_inz * zq;
        });
        // (P r_x)[p_e]: the pivot columns of the P buffer are as loaded and P is symmetric; xb holds the whole of r_x
        stage_y(yb, zrow ? wgt * qp : 0.0);
        wv_sync();
        const double hq = wv_mv_cols<NX>(A, m, yb, lane) + wv_mv_cols<NX>(Pm, n, xb, lane);
        if (xm && peq >= 0) xb2[peq] = hq - fk;
        wv_sync();
        const double muc = wv_mv_cols<NX>(Rp, neq, xb2, lane);      // lane p_e: mu_e = sum_i B_1^-1[i][e] g_i  (g of a dropped row is 0)
        wv_sync();
        if (xm && peq >= 0) xb2[peq] = muc;
        wv_sync();
        const double mue = eqi >= 0 ? xb2[eqi] : 0.0;               // (a dropped row kept its 0)

        // r_y
        double ry = (rk == RK_EQ) ? mue : d;      // equalities: the multiplier; eliminated rows: d = 0
        for_cones([&](int r0, int r1) {
            if (lane_bcast_i(rk, r0) != RK_SOCB) return;
            const bool tail = lane > r0 && lane < r1;
            const double nz = lane_bcast(c_nz, r0), d0 = lane_bcast(d, r0), zdn = wave_sum(tail ? v * d : 0.0) / nz;
            const double eyd = (d0 + zdn) * M_SQRT1_2, esd = (d0 - zdn) * M_SQRT1_2;      // (as the first loop computed them from the same column of D)
            const double lam = lane_bcast(c_lam, r0), zq = lane_bcast(c_zq, r0), rhoy = lane_bcast(mue, r0);
            const int ce = lane_bcast_i(eqi, r0);
            const double eyq = lane_bcast_i(pcl, ce) >= 0 ? eyd : 0.0;      // a_y . r_x = e_y . d (the equality; a dropped row is flagged anyway)
            const double q0 = M_SQRT2 * eyq - zq, esq = (q0 - zq) * M_SQRT1_2, il = 1.0 / (1 - lam);
            const double cy = rhoy - il * (eyd - lam * eyq), cs = esd - il * (esd - lam * esq);
            const double k0 = (cy + cs) * M_SQRT1_2, kz = (cy - cs) * M_SQRT1_2;
            if (tail) ry = il * (d - lam * qv) + kz * (v * c_inz);
            if (lane == r0) ry = il * (d - lam * q0) + k0;
        });

        // outputs in the boundary convention: dA_eval = [-dA.data, db[b_idx]], dq_eval = [dc, 0]
        if (W.rec) {      // record mode: (r_y, r_tau = 0, r_x) of the pair; k_param_grad behind the launch evaluates the entries, dP's among them
            double *const rec = W.rec + kk * W.srk + (long)inst * W.rpitch;
            if (ym) rec[lane] = ry;
            if (xm) rec[m + 1 + lane] = rx;
            if (lane == 0) rec[m] = 0.0;
        } else {
            wv_sync();
            stage_x(xb, rx); stage_x(xb2, xv);
            stage_y(yb, ry); stage_y(yb2, yv);
            wv_sync();
            double *const dArow = dAo + kk * W.sAk + (long)inst * nnz, *const dProw = W.dP + kk * W.sPk + (long)inst * nnz_p;
            for (int e = lane; e < nnz; e += 64) {
                const int i = T.rowidx[e], j = T.colidx[e], jc = j < n ? j : 0;
                const double va = ce_dA_entry(xb2[jc], yb[i], yb2[i], xb[jc]);
                dArow[e] = j < n ? va : -yb[i];
            }
            // dP = -sym(r_x x^T) through the structure; a one-triangle entry stands for both matrix entries and takes both shares (k_backward_ns<QP, MANY>'s epilogue)
            for (int e = lane; e < nnz_p; e += 64) {
                const int i = W.prow[e], j = W.pcol[e];
                const double va = ce_dP_entry(xb[i], xb2[j], xb[j], xb2[i]);
                dProw[e] = (W.p_tri && i != j) ? 2.0 * va : va;
            }
        }
        if (lane <= n) dqo[kk * W.sqk + lane * sdqk + (long)inst * sdqb] = xm ? -rx : 0.0;
        if (lane == 0 && adj_status) adj_status[kk * W.sak + (long)inst] = flags;      // (bit 4: a dropped row or variable; the dropped-variable answer stands)
    }
}

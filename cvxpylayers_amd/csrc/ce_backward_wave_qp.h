// ce_backward_wave_qp.h -- k_bwd_wave_qp: the adjoint of a SMALL template with a QUADRATIC objective inside the kernels, one instance per wave (opt-in:
// ce_vjp_qp_wave).
//
// The system and the answer are k_backward_ns<..., QP, MANY>'s at K = 1 (ce_backward_ns.h), r_tau pinned to 0:
//        (H + P) r_x - B^T mu = f,   B r_x = d_B,        H = sum_c theta_c (A_z^T A_z - a_z a_z^T)  over the boundary cones,   B = the neq equality rows,
// solved by the null-space elimination of k_bwd_wave (ce_backward_wave.h), whose stages 1-5, placement, classification of rows and cones, kink rules, f, d_B,
// r_y, dq = -r_x and dA row are RESTATED here unchanged (sharing them through helpers would have to leave bwd_wave.o's device code byte-identical; a restated
// kernel cannot touch it -- k_newton_wave's choice).  What P adds:
//   load      P is a third dense LDS matrix (n rows of NX + 1) behind A and R | B_1^-1, zeroed with them, scattered from the instance's row of P_vals through
//             the handle's (row, column) arrays: a one-triangle entry fills (i, j) and (j, i), a full-structure entry its own slot (k_fwd_wave_qp's convention).
//   stage 2   while the eliminated rows c1[] are registers: every row of P through transform() (W = P Z in the free columns, the pivot columns keep P), then every
//             FREE column b of W, read with lane = row, through the same transform(): that is column b of Z^T P Z, by symmetry its row b with lane = column, and
//             lane n ends with -(Z^T P x_p)_b on its own -- the reduced right-hand side's share, so no further transform of a right-hand-side column is needed.
//             Written back in place (free rows of column b; column NX of row b): c1[] and G[] are never live together, k_bwd_wave's register budget, every row.
//   stage 3   G[a] starts from row a of that buffer (lane n: -(Z^T P x_p)_a), the Gram of H's weighted rows is accumulated onto it; dg, the diagonal the sweep's
//             rank test compares against, is Z^T (H + P) Z's.  No weighted row and neq = 0: the reduced Hessian is P alone.
//   stage 5   g = ((H + P) r_x - f)[piv]: (P r_x)[p_e] is one more wv_mv_cols over the P buffer with the staged r_x -- pivot columns untouched, P symmetric.
//   output    dP (B, nnz_p) batch-major: entry k = ce_dP_entry(r_x[i], x[j], r_x[j], x[i]), doubled off the diagonal of a one-triangle structure.
//   flags     k_backward_ns<QP>'s: neq > n is status 4 with zero dA, dq, dP; a dropped equality row or variable sets bit 4 and the dropped-variable answer stands.
//             No re-solve list, no LSQR (none has a P term): bit 8 is never set, and the factor mode of dA (which the re-solve arms) does not exist here.
// LDS is written and read by the owning wave only (wv_sync(), no workgroup barrier).  Every loop is bounded by n, m, neq, nnz, the cone count or a compile-time count.
#pragma once
#include "ce_common.h"
#include "ce_wave_helpers.h"
#include "ce_forward_wave.h"     // wv_sync, fold, lane_bcast, wv_max, wv_mv_cols, wv_mv_rows: the one-wave building blocks, stated once
#include "ce_backward_wave.h"    // lane_bcast_i, bw_recip
#include "ce_dA_entry.h"         // ce_dA_entry, ce_dP_entry: shared with k_backward_ns
#include "ce_lds_bwd_wave_qp.h"  // bwd_wave_qp_lds_doubles: the total of the carve below

template <int NX, int MY, int WPS>
__global__ void __launch_bounds__(64, WPS)
k_bwd_wave_qp(DevT T, const double *__restrict__ Avals, const double *__restrict__ Pvals, int nnz_p, const int *__restrict__ pri, const int *__restrict__ pci, int p_tri,
              const double *__restrict__ xg, const double *__restrict__ yg, const double *__restrict__ sg, const double *__restrict__ dxg, const double *__restrict__ dyg,
              double *__restrict__ dAo, double *__restrict__ dqo, long sdqk, long sdqb, double *__restrict__ dPo, int *__restrict__ adj_status) {
    static_assert(NX <= 32 && MY <= 64 && 64 % NX == 0 && 64 % MY == 0 && NX >= 8 && NX < MY, "k_bwd_wave_qp: one lane per row, one per column and one for the right-hand side");
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int LD = NX + 1, NG = NX / 8;
    const int lane = threadIdx.x;
    const size_t inst = blockIdx.x;
    const int n = T.n, m = T.m, z = T.z, zl = T.z + T.l, nq = T.nq, nnz = T.nnz_aug;
    double *A = sm, *Rp = A + m * LD, *Pm = Rp + NX * LD, *xb = Pm + n * LD, *xb2 = xb + NX, *yb = xb2 + NX, *yb2 = yb + MY;
    int *erow = (int *)(yb2 + MY);
    const bool xm = lane < n, ym = lane < m;
    const unsigned long long lt = (1ull << lane) - 1ull;

    int qe = 0;      // first row behind the second-order cone this lane's row belongs to (k_fwd_wave's walk)
    if (ym && lane >= zl) qe = T.qoff[T.rowcone[lane] + 1];
    auto for_cones = [&](auto &&f) {
        int r0 = zl;
        for (int c = 0; c < nq; c++) { const int r1 = __builtin_amdgcn_readlane(qe, r0); f(r0, r1); r0 = r1; }
    };
    auto stage_x = [&](double *buf, double v) { if (lane < NX) buf[lane] = v; };
    auto stage_y = [&](double *buf, double v) { if (lane < MY) buf[lane] = v; };

    // ---------------------------------------------------------------- load: A = -A_cvx dense through the template's structure (b is not needed: r_tau is pinned),
    //      P dense through its own (k_fwd_wave_qp's convention: a one-triangle entry fills both slots, a full-structure entry its own)
    for (int i = lane; i < (m + NX + n) * LD; i += 64) A[i] = 0.0;      // (A, R and P are contiguous)
    double v = 0.0, d = 0.0;
    if (ym) { v = yg[inst * m + lane] - sg[inst * m + lane]; d = dyg[inst * m + lane]; }
    const double dxv = xm ? dxg[inst * n + lane] : 0.0;
    wv_sync();
    {
        const double *vals = Avals + inst * nnz;
        for (int k = lane; k < nnz; k += 64) {
            const double a = vals[k]; const int r = T.rowidx[k], c = T.colidx[k];
            if (c < n) A[r * LD + c] = -a;
        }
        const double *pv = Pvals + inst * (size_t)nnz_p;
        for (int k = lane; k < nnz_p; k += 64) {
            const double a = pv[k]; const int r = pri[k], c = pci[k];
            Pm[r * LD + c] = a;
            if (p_tri && r != c) Pm[c * LD + r] = a;
        }
    }

    // ---------------------------------------------------------------- classify and d = DPi(v) dy in one pass; u: the row's weight in f = dx + A^T u
    int rk = RK_FREE;
    bool trow = false;                               // the t-row of a boundary cone
    double u = 0.0, wgt = 0.0;                       // weight of the row in H: theta (z-rows of a boundary cone), -theta (its t-row slot: a_z), else 0
    double c_lam = 0.0, c_inz = 0.0, c_eyd = 0.0, c_esd = 0.0;      // of the boundary cone this row belongs to
    if (lane < zl) { const bool eq = lane < z || v > 0; rk = eq ? RK_EQ : RK_FREE; if (!eq) d = 0.0; }
    for_cones([&](int r0, int r1) {
        const bool in = lane >= r0 && lane < r1, tail = lane > r0 && lane < r1;
        const double t0 = lane_bcast(v, r0), h0 = lane_bcast(d, r0);
        const double nz = sqrt(wave_sum(tail ? v * v : 0.0)), zh = wave_sum(tail ? v * d : 0.0);
        int kind;
        if (r1 - r0 == 1) kind = t0 >= 0 ? 0 : 1;
        else if (nz <= t0) kind = 0; else if (nz <= -t0) kind = 1; else kind = 2;
        if (kind == 0) { if (in) rk = RK_EQ; }
        else if (kind == 1) { if (in) { rk = RK_FREE; d = 0.0; } }
        else {
            const double lam = (t0 + nz) / (2 * nz), i2n = 1.0 / (2 * nz), cz = t0 * zh / (nz * nz), inz = 1.0 / nz;
            const double di = tail ? (v * h0 + (t0 + nz) * d - v * cz) * i2n : 0.0;
            const double zd = wave_sum(tail ? v * di : 0.0);
            const double d0 = (nz * h0 + zh) * i2n, zdn = zd / nz, eyd = (d0 + zdn) * M_SQRT1_2, esd = (d0 - zdn) * M_SQRT1_2;
            const double il = 1.0 / (1 - lam), th = lam / (1 - lam);
            const double k0c = (esd * (1 - il) - eyd * il) * M_SQRT1_2, kzc = (-esd * (1 - il) - eyd * il) * M_SQRT1_2;
            if (tail) { d = di; u = fma(il, di, v * inz * kzc); wgt = th; }
            if (lane == r0) { d = d0; u = fma(il, d0, k0c); wgt = -th; trow = true; }
            if (in) { rk = RK_SOCB; c_lam = lam; c_inz = inz; c_eyd = eyd; c_esd = esd; }
        }
    });

    // ---------------------------------------------------------------- numbering of the equality rows: the rows in order, then one e_y row per boundary cone
    const bool isEq = ym && rk == RK_EQ;
    const unsigned long long balE = __ballot(isEq), balT = __ballot(trow);
    const int base = __popcll(balE), neq = base + __popcll(balT);
    const int eqi = isEq ? __popcll(balE & lt) : (trow ? base + __popcll(balT & lt) : -1);
    if (neq > n) {      // more active rows than variables: rank deficient by counting (zero gradient, status 4 as k_backward_ns<QP>: no list, no re-solve)
        double *const dArow = dAo + inst * nnz, *const dProw = dPo + inst * (size_t)nnz_p;
        for (int k = lane; k < nnz; k += 64) dArow[k] = 0.0;
        for (int k = lane; k < nnz_p; k += 64) dProw[k] = 0.0;
        if (lane <= n) dqo[lane * sdqk + (long)inst * sdqb] = 0.0;
        if (lane == 0 && adj_status) adj_status[inst] = 4;
        return;
    }
    wv_sync();      // (the scatters of A and P)

    // ---------------------------------------------------------------- f = dx + A^T u (all rows of the boundary cones at once, the t-rows still a_0)
    stage_y(yb, u); stage_y(yb2, v);
    if (eqi >= 0) erow[eqi] = lane;
    wv_sync();
    double fx;
    { const double a = wv_mv_cols<NX>(A, m, yb, lane); fx = xm ? dxv + a : 0.0; }
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

    // ---------------------------------------------------------------- 1. [B | d_B] in registers: lane = column, lane n = the right-hand side, row e = c1[e]
    double c1[NX];
    double rtl = 0.0;                              // lane e: rank tolerance of equality row e (CE_RANK_TOL x its largest entry as loaded)
    {
        const int erl = lane < neq ? erow[lane] : 0;
        const double dbv = trow ? c_eyd : d;      // right-hand side of the row's equality
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
    // v_readlane and one FMA; the scaled pivot row carries 1 + 1/p in the pivot column, so that the pivot columns end as B_1^-1 (k_backward_ns's one-wave scheme).
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
            } else { c1[e] = 0.0; flags |= 4; }      // redundant equality row: dropped (mu_e = 0), the instance is flagged
        }
    });
    const bool fr = xm && cfr;
    const unsigned fmask = (unsigned)__ballot(fr);
    // R (free columns), B_1^-1 (pivot columns) and d~ (column NX) parked in LDS for x_piv and mu
    static_for<NX>([&](auto ec) {
        constexpr int e = decltype(ec)::value;
        if (e < neq && lane <= n) Rp[e * LD + (xm ? lane : NX)] = c1[e];
    });

    // ---------------------------------------------------------------- 2. null-space transform, lane = column, against the register rows:
    //      a~[j] = a[j] - sum_e a[p_e] R[e][j] (free j);  lane n ends with -t = -sum_e a[p_e] d~_e.  The pivot entries of a row stay as loaded.
    //      The entries a[p_e] are gathered once per row, lane e <- lane p_e (one ds_bpermute pair; a dropped row reads lane 0 against a zero register row), and
    //      then read by v_readlane at a constant lane: no wave-uniform array of pivot columns (as scalars it spilled to VGPR lanes at NX = 32).
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
    // Z^T P Z, which is also its row b with lane = column; lane n ends with -sum_e W[p_e][b] d~_e = -(Z^T P x_p)_b, the right-hand side of that row, on its own.
    // In place: the free rows of column b, and column NX of row b.  No later column reads either slot, and c1[] and G[] are never live together.
    for (unsigned fm = fmask; fm; fm &= fm - 1) {
        const int b = __builtin_ctz(fm);
        const double zn = transform(xm ? Pm[lane * LD + b] : 0.0);
        if (fr) Pm[lane * LD + b] = zn;
        if (lane == n) Pm[b * LD + NX] = zn;
    }
    wv_sync();

    // ---------------------------------------------------------------- 3. reduced Hessian in registers: G[a] (lane b) = sum_k w_k a~_k[a] a~_k[b], lane n: the
    //      right-hand side Z^T f - sum_k w_k t_k a~_k.  Pivot rows and columns stay zero.
    //      (For n not a multiple of 8 the groups of eight cover register rows a >= n: row n picks up the right-hand-side lane's -t w and is swept along with the
    //      rest.  Harmless -- such a row is never a pivot row, its column entries in the rows < n are zero, and r_x is read from the free lanes alone.)
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
    double dg = 0.0;      // lane a: the original diagonal entry of row a
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

    // ---------------------------------------------------------------- 5. x_piv = d~ - R x_free;  q_k = a_k . r_x = t_k + a~_k . x_free for the weighted rows
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
    // per boundary cone: a_z . r_x = z-hat . (A_z r_x);  q'_i = q_i - z-hat_i (a_z . r_x), so that H r_x = sum over the z-rows of theta a_i q'_i needs no a_z
    double c_zq = 0.0, qp = 0.0;
    for_cones([&](int r0, int r1) {
        if (lane_bcast_i(rk, r0) != RK_SOCB) return;
        const bool in = lane >= r0 && lane < r1, tail = lane > r0 && lane < r1;
        const double zq = wave_sum(tail ? v * qv : 0.0) * lane_bcast(c_inz, r0);
        if (in) c_zq = zq;
        if (tail) qp = qv - v * c_inz * zq;
    });
    // g = ((H + P) r_x - f)[piv] by equality, mu = B_1^-T g.  (P r_x)[p_e]: the pivot columns of the P buffer are as loaded and P is symmetric
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

    // ---------------------------------------------------------------- r_y
    double ry = (rk == RK_EQ) ? mue : d;      // equalities: the multiplier; eliminated rows: d = 0
    for_cones([&](int r0, int r1) {
        if (lane_bcast_i(rk, r0) != RK_SOCB) return;
        const bool tail = lane > r0 && lane < r1;
        const double lam = lane_bcast(c_lam, r0), eyd = lane_bcast(c_eyd, r0), esd = lane_bcast(c_esd, r0), zq = lane_bcast(c_zq, r0), rhoy = lane_bcast(mue, r0);
        const int ce = lane_bcast_i(eqi, r0);
        const double eyq = lane_bcast_i(pcl, ce) >= 0 ? eyd : 0.0;      // a_y . r_x = e_y . d (the equality; a dropped row is flagged anyway)
        const double q0 = M_SQRT2 * eyq - zq, esq = (q0 - zq) * M_SQRT1_2, il = 1.0 / (1 - lam);
        const double cy = rhoy - il * (eyd - lam * eyq), cs = esd - il * (esd - lam * esq);
        const double k0 = (cy + cs) * M_SQRT1_2, kz = (cy - cs) * M_SQRT1_2;
        if (tail) ry = il * (d - lam * qv) + kz * (v * c_inz);
        if (lane == r0) ry = il * (d - lam * q0) + k0;
    });

    // ---------------------------------------------------------------- outputs in the boundary convention: dA_eval = [-dA.data, db[b_idx]], dq_eval = [dc, 0]
    double *const dArow = dAo + inst * nnz, *const dProw = dPo + inst * (size_t)nnz_p;
    wv_sync();
    stage_x(xb, rx); stage_x(xb2, xm ? xg[inst * n + lane] : 0.0);
    stage_y(yb, ry); stage_y(yb2, ym ? yg[inst * m + lane] : 0.0);
    wv_sync();
    for (int k = lane; k < nnz; k += 64) {
        const int i = T.rowidx[k], j = T.colidx[k], jc = j < n ? j : 0;
        const double va = ce_dA_entry(xb2[jc], yb[i], yb2[i], xb[jc]);
        dArow[k] = j < n ? va : -yb[i];
    }
    // dP = -sym(r_x x^T) through the structure; a one-triangle entry stands for both matrix entries and takes both shares (k_backward_ns<QP, MANY>'s epilogue)
    for (int k = lane; k < nnz_p; k += 64) {
        const int i = pri[k], j = pci[k];
        const double va = ce_dP_entry(xb[i], xb2[j], xb[j], xb2[i]);
        dProw[k] = (p_tri && i != j) ? 2.0 * va : va;
    }
    if (lane <= n) dqo[lane * sdqk + (long)inst * sdqb] = xm ? -rx : 0.0;
    if (lane == 0 && adj_status) adj_status[inst] = flags;      // (bit 4: a dropped row or variable; the dropped-variable answer stands -- no LSQR has a P term)
}

// ce_forward_wave.h -- k_fwd_wave: the forward solve of a SMALL template, one instance per wave (opt-in: ce_solve_wave).
//
// Every other forward kernel gives an instance a workgroup of 256 or 512 threads and steps through its iteration with workgroup barriers; for a template of a few
// tens of rows the threads idle between the barriers and a CU holds three instances.  Here an instance is ONE wave (a 64-thread workgroup): no other wave to wait
// for, so no workgroup barrier anywhere -- an instance that stops at iteration 50 frees its slot beside a neighbour that runs 1500 -- and what is resident per
// CU is bounded by registers and LDS per wave alone.
//
// Placement (n <= NX <= 32, m <= MY <= 64):
//   * every vector lives in REGISTERS, one element per lane: lane j < n holds entry j of the x part, lane i < m entry i of the y part (both in the same lane), the
//     tau entry is wave-uniform.  Lanes beyond n / m hold 0.0, so dots and norms are plain wave reductions (DPP, ce_common.h wave_reduce_dpp).  The Anderson
//     history (x_prev, f_prev, f_save, w_prev) is four more such vectors.
//   * A-hat (m x (NX + 1)) and G = (rho_x I + A-hat^T R_y A-hat)^-1 (n x (NX + 1)) live in this wave's LDS, zero padded; the odd stride makes both the row-per-lane
//     product (A-hat v) and the column-per-lane product (A-hat^T y, G t) conflict free.  All 64 lanes work on either product: 64 / MY lanes share a row, 64 / NX a
//     column, and fold their partial sums by DPP / v_permlane swaps (fold<>).  The vector operand is staged through LDS (xb, xb2, yb, yb2).
//   * a second-order cone needs its segment's norm: one wave reduction per cone, the cone's extent read from the lanes (qe).
// LDS is written and read by the same wave only: wv_sync() orders the accesses (a fence and a wave barrier, no s_barrier).
//
// Algorithm: oracle/cone_oracle.c solve_one, statement by statement as the size-generic k_forward (ce_forward_generic.h) states it.
#pragma once
#include "ce_common.h"
#include "ce_wave_helpers.h"
#include "ce_lds_fwd_wave.h"    // fwd_wave_lds_doubles: the total of the carve below

// orders this wave's LDS writes before its later LDS reads (other lanes' data): the one-wave counterpart of __syncthreads()
__device__ __forceinline__ void wv_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// all-reduce over the lanes that share (lane % W), W in {8, 16, 32, 64}; MAX on non-negative values only.  row_ror:8, then gfx950's v_permlane16_swap /
// v_permlane32_swap with both operands the same register (ce_common.h colsum_rows): no LDS crossbar
template <int W, bool MAX>
__device__ __forceinline__ double fold(double v) {
    auto op = [](double a, double b) { return MAX ? fmax(a, b) : a + b; };
    if constexpr (W <= 8) v = op(v, dpp_mov<0x128>(v));
    if constexpr (W <= 16) {
        const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
        const auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false), b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        v = op(__hiloint2double((int)b[0], (int)a[0]), __hiloint2double((int)b[1], (int)a[1]));
    }
    if constexpr (W <= 32) {
        const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
        const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false), b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        v = op(__hiloint2double((int)b[0], (int)a[0]), __hiloint2double((int)b[1], (int)a[1]));
    }
    return v;
}
// the value lane `src` holds (src wave-uniform), in every lane
__device__ __forceinline__ double lane_bcast(double v, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wv_max(double v) { return wave_reduce_dpp<true>(v); }      // (non-negative values)

// out[j] = sum_{i < rows} Mat[i][j] v[i], j = lane % NX: 64 / NX lanes share a column and take every (64 / NX)-th row.  Every lane gets its column's sum.
template <int NX>
__device__ __forceinline__ double wv_mv_cols(const double *Mat, int rows, const double *v, int lane) {
    constexpr int LD = NX + 1, CH = 64 / NX;
    const int j = lane % NX, ch = lane / NX;
    double a0 = 0, a1 = 0;
    for (int i = ch; i < rows; i += 2 * CH) {
        a0 = fma(Mat[i * LD + j], v[i], a0);
        if (i + CH < rows) a1 = fma(Mat[(i + CH) * LD + j], v[i + CH], a1);
    }
    return fold<NX, false>(a0 + a1);
}
// out[i] = sum_{j < cols} Mat[i][j] v[j], i = lane % MY (rows beyond `rows` read row 0: the caller masks them): 64 / MY lanes share a row.
template <int NX, int MY>
__device__ __forceinline__ double wv_mv_rows(const double *Mat, int rows, int cols, const double *v, int lane) {
    constexpr int LD = NX + 1, CH = 64 / MY;
    const int i = lane % MY, ch = lane / MY;
    const double *r = Mat + (i < rows ? i : 0) * LD;
    double a0 = 0, a1 = 0;
    for (int j = ch; j < cols; j += 2 * CH) {
        a0 = fma(r[j], v[j], a0);
        if (j + CH < cols) a1 = fma(r[j + CH], v[j + CH], a1);
    }
    return fold<MY, false>(a0 + a1);
}

template <int NX, int MY, int WPS>
__global__ void __launch_bounds__(64, WPS)
k_fwd_wave(DevT T, ce_settings S, const double *__restrict__ Avals, const double *__restrict__ qv, long sqk, long sqb,
           double *xo, double *yo, double *so, int *__restrict__ iters_o, int *__restrict__ status_o, double *__restrict__ resid_o) {
    static_assert(NX <= 32 && MY <= 64 && 64 % NX == 0 && 64 % MY == 0 && NX >= 8, "k_fwd_wave: one lane per row, whole groups of lanes per column");
    extern __shared__ __attribute__((aligned(16))) double sm[];
    constexpr int LD = NX + 1;
    const int lane = threadIdx.x;
    const size_t inst = blockIdx.x;
    const int n = T.n, m = T.m, l = n + m + 1, z = T.z, zl = T.z + T.l, nq = T.nq;
    double *A = sm, *G = A + m * LD, *xb = G + n * LD, *xb2 = xb + NX, *yb = xb2 + NX, *yb2 = yb + MY;
    const bool xm = lane < n, ym = lane < m;

    // first row behind the second-order cone this lane's row belongs to: the cones are walked from the lanes (for_cones), no table in the loop
    int qe = 0;
    if (ym && lane >= zl) qe = T.qoff[T.rowcone[lane] + 1];
    auto for_cones = [&](auto &&f) {
        int r0 = zl;
        for (int c = 0; c < nq; c++) { const int r1 = __builtin_amdgcn_readlane(qe, r0); f(r0, r1); r0 = r1; }
    };
    auto stage_x = [&](double *buf, double v) { if (lane < NX) buf[lane] = v; };
    auto stage_y = [&](double *buf, double v) { if (lane < MY) buf[lane] = v; };
    auto ATv = [&](const double *v) { const double a = wv_mv_cols<NX>(A, m, v, lane); return xm ? a : 0.0; };
    auto Gv = [&](const double *v) { const double a = wv_mv_cols<NX>(G, n, v, lane); return xm ? a : 0.0; };
    auto Av = [&](const double *v) { const double a = wv_mv_rows<NX, MY>(A, m, n, v, lane); return ym ? a : 0.0; };

    // ---------------------------------------------------------------- load: one gather through the template's CSC structure (lanes along the instance's value row)
    for (int i = lane; i < (m + n) * LD; i += 64) A[i] = 0.0;      // (A and G are contiguous)
    if (lane < MY) yb[lane] = 0.0;
    wv_sync();
    {
        const double *vals = Avals + inst * T.nnz_aug;
        for (int k = lane; k < T.nnz_aug; k += 64) {
            const double v = vals[k]; const int r = T.rowidx[k], c = T.colidx[k];
            if (c < n) A[r * LD + c] = -v;      // solver sees A = -A_cvx (diffcp_if.py:65)
            else yb[r] = v;                     // b = b_cvx          (diffcp_if.py:66)
        }
    }
    wv_sync();
    double bv = ym ? yb[lane] : 0.0;
    double cv = xm ? qv[lane * sqk + (long)inst * sqb] : 0.0;
    double Dv = 1.0, Ev = 1.0;
    const double nrm_b0 = wv_max(fabs(bv)), nrm_c0 = wv_max(fabs(cv));

    // ---------------------------------------------------------------- equilibration (SCS normalize)
    double sigma = 1.0;
    if (S.normalize) {
        for (int pass = 0; pass < NUM_RUIZ_PASSES + NUM_L2_PASSES; pass++) {
            const bool l2 = pass >= NUM_RUIZ_PASSES;
            double rn, cn;
            {
                constexpr int CH = 64 / MY;
                const int i = lane % MY, ch = lane / MY;
                const double *r = A + (i < m ? i : 0) * LD;
                double a = 0;
                for (int j = ch; j < n; j += CH) { const double v = r[j]; a = l2 ? fma(v, v, a) : fmax(a, fabs(v)); }
                a = l2 ? fold<MY, false>(a) : fold<MY, true>(a);
                rn = l2 ? sqrt(a) : a;
            }
            {
                constexpr int CH = 64 / NX;
                const int j = lane % NX, ch = lane / NX;
                double a = 0;
                for (int i = ch; i < m; i += CH) { const double v = A[i * LD + j]; a = l2 ? fma(v, v, a) : fmax(a, fabs(v)); }
                a = l2 ? fold<NX, false>(a) : fold<NX, true>(a);
                cn = l2 ? sqrt(a) : a;
            }
            double tvv = (lane < zl) ? 1.0 / sqrt(clamp_scale(rn)) : rn;      // cone rows: raw norm, averaged over the cone so the scaled cone is still the cone
            for_cones([&](int r0, int r1) {
                const bool in = lane >= r0 && lane < r1;
                double a = wave_sum(in ? tvv : 0.0);
                a = 1.0 / sqrt(clamp_scale(a / (r1 - r0)));
                if (in) tvv = a;
            });
            double et = 1.0 / sqrt(clamp_scale(cn));
            if (!ym) tvv = 1.0;
            if (!xm) et = 1.0;
            wv_sync();
            stage_y(yb, tvv); stage_x(xb, et);
            wv_sync();
            for (int idx = lane; idx < m * LD; idx += 64) { const int i = idx / LD, j = idx - i * LD; if (j < n) A[idx] *= yb[i] * xb[j]; }
            wv_sync();
            Dv *= tvv; Ev *= et;
        }
        bv *= Dv; cv *= Ev;
        sigma = 1.0 / clamp_scale(fmax(wv_max(fabs(bv)), wv_max(fabs(cv))));
        bv *= sigma; cv *= sigma;
    }

    double scale = S.scale;
    const double rho_x = S.rho_x, rtau = TAU_FACTOR, alpha = S.alpha;
    double hg = 0, dyl = 0;                         // h . g ; 1 / r_y of this lane's row
    double gx = 0, gy = 0, phix = 0, phiy = 0;      // g = K^-1 h ; the functional giving the tau-tilde numerator

    // ---- (re)factor: G = (rho_x I + A^T Dy A)^{-1}, g, h.g, phi   (wave-uniform control flow)
    auto refactor = [&]() {
        auto dyv = [&](int i) -> double { return (i < z) ? ZERO_CONE_FACTOR * scale : scale; };
        dyl = dyv(lane);
        wv_sync();
        for (int idx = lane; idx < n * n; idx += 64) {
            const int a = idx / n, b2 = idx - a * n;
            double acc0 = 0, acc1 = 0; int i = 0;
            for (; i + 1 < m; i += 2) {
                acc0 = fma(A[i * LD + a] * dyv(i), A[i * LD + b2], acc0);
                acc1 = fma(A[(i + 1) * LD + a] * dyv(i + 1), A[(i + 1) * LD + b2], acc1);
            }
            if (i < m) acc0 = fma(A[i * LD + a] * dyv(i), A[i * LD + b2], acc0);
            G[a * LD + b2] = acc0 + acc1 + (a == b2 ? rho_x : 0.0);
        }
        wv_sync();
        for (int k = 0; k < n; k++) {      // in-place Gauss-Jordan inversion (SPD: no pivoting needed); column and row k staged in xb / xb2
            if (xm) { xb[lane] = G[lane * LD + k]; xb2[lane] = G[k * LD + lane]; }
            wv_sync();
            const double pinv = 1.0 / xb2[k];
            for (int idx = lane; idx < n * n; idx += 64) {
                const int i = idx / n, j = idx - i * n;
                double v;
                if (i == k) v = (j == k) ? pinv : xb2[j] * pinv;
                else if (j == k) v = -xb[i] * pinv;
                else v = fma(-xb[i] * pinv, xb2[j], G[i * LD + j]);
                G[i * LD + j] = v;
            }
            wv_sync();
        }
        stage_y(yb, dyl * bv);
        wv_sync();
        const double atb = ATv(yb);                        // A^T Dy b
        stage_x(xb, cv - atb); stage_x(xb2, cv + atb);    // rhs of g_x ; k, for phi
        wv_sync();
        gx = Gv(xb);
        const double Gk = Gv(xb2);
        wv_sync();
        stage_x(xb, gx); stage_x(xb2, Gk);
        wv_sync();
        const double agx = Av(xb), aGk = Av(xb2);
        gy = ym ? dyl * (agx + bv) : 0.0;
        phiy = bv - aGk; phix = rho_x * Gk;
        hg = wave_sum(bv * gy + cv * gx);
        wv_sync();
    };

    refactor();
    double wx = 0, wy = 0, w_t = 1.0;      // cold start
    double phiw = 0;                       // phi . w (z part)
    if (S.warm_start) {   // u = (x^, y^, 1), v = (0, s^, 0); w = u + R^-1 v  (see k_fwd2)
        const double x0 = xm ? xo[inst * n + lane] : 0.0, y0 = ym ? yo[inst * m + lane] : 0.0, s0 = ym ? so[inst * m + lane] : 0.0;
        const bool bad = !(fabs(x0) < 1e300) || !(fabs(y0) < 1e300) || !(fabs(s0) < 1e300);
        if (wv_max(bad ? 1.0 : 0.0) == 0.0) {      // a non-finite point starts cold
            wx = xm ? sigma * x0 / Ev : 0.0;
            wy = ym ? sigma * y0 / Dv + sigma * Dv * s0 * dyl : 0.0;
            phiw = wave_sum(phix * wx + phiy * wy);
        }
    }

    int status = 0, iter = 0, last_scale_iter = 0, n_log = 0;
    double sum_log = 0, res_pri = NAN, res_dual = NAN, gap = NAN;
    double tau = 0, kap = 0, ctx = 0, bty = 0;
    double utx = 0, uty = 0, ut_t = 0, ux = 0, uy = 0, u_t = 0;

    // Anderson acceleration of the iteration map w -> F(w): type I, ONE secant pair, residual safeguard, switched off after AA_MAX_REJECT rejections -- the algorithm
    // of k_fwd2 / k_forward and of the oracle with aa_mem = 1.  The four history vectors are registers (x part, y part, tau entry).
    bool aa_on = S.acceleration_lookback > 0, aa_pending = false, aa_stale = false;
    const int aa_int = S.acceleration_interval > 0 ? S.acceleration_interval : 10;
    int aa_iter = 0, aa_rej = 0;
    double aa_normg = 0, aa_hs = 1.0;     // |g| before the step ; factor the stored history has to be scaled by (the renormalisations of w since it was stored)
    double xpx = 0, xpy = 0, xpt = 0, fpx = 0, fpy = 0, fpt = 0, fsx = 0, fsy = 0, fst = 0, wpx = 0, wpy = 0, wpt = 0;

    for (iter = 0; iter < S.max_iters; iter++) {
        const bool check = (iter % CONVERGED_INTERVAL) == 0;
        if (aa_on) {
            bool w_changed = false;
            if (aa_pending) {      // safeguard: residual of the map at the accelerated point against the residual before the step
                const double dx = wpx - wx, dy = wpy - wy, dt = wpt - w_t;
                const double rs = wave_sum(fma(dx, dx, dy * dy)) + dt * dt;
                if (!(sqrt(rs) <= aa_normg)) {
                    wx = fsx * aa_hs; wy = fsy * aa_hs; w_t = fst * aa_hs;
                    aa_iter = 0; w_changed = true;
                    if (++aa_rej >= AA_MAX_REJECT) aa_on = false;
                }
                aa_pending = false;
            }
            if (aa_on && iter > 0 && iter % aa_int == 0 && !aa_stale) {      // (aa_stale: w_prev predates a rescale)
                if (aa_iter > 0) {
                    double rr[5] = {0, 0, 0, 0, 0};
                    auto acc = [&](double xv, double fv, double xp0, double fp0) {
                        const double gv = xv - fv, xp = xp0 * aa_hs, fp = fp0 * aa_hs, sv = xv - xp, yv = gv - (xp - fp);
                        rr[0] = fma(sv, sv, rr[0]); rr[1] = fma(yv, yv, rr[1]); rr[2] = fma(sv, yv, rr[2]); rr[3] = fma(sv, gv, rr[3]); rr[4] = fma(gv, gv, rr[4]);
                    };
                    acc(wpx, wx, xpx, fpx); acc(wpy, wy, xpy, fpy);
#pragma unroll
                    for (int k = 0; k < 5; k++) rr[k] = wave_sum(rr[k]);
                    {      // the tau entry, once
                        const double xv = wpt, fv = w_t, gv = xv - fv, xp = xpt * aa_hs, fp = fpt * aa_hs, sv = xv - xp, yv = gv - (xp - fp);
                        rr[0] = fma(sv, sv, rr[0]); rr[1] = fma(yv, yv, rr[1]); rr[2] = fma(sv, yv, rr[2]); rr[3] = fma(sv, gv, rr[3]); rr[4] = fma(gv, gv, rr[4]);
                    }
                    const double mm = rr[2] + 1e-8 * sqrt(rr[0]) * sqrt(rr[1]), gam = rr[3] / mm;
                    const bool ok = fabs(mm) > 1e-300 && fabs(gam) < 1e10;
                    const double opx = fpx * aa_hs, opy = fpy * aa_hs, opt = fpt * aa_hs;
                    xpx = wpx; xpy = wpy; xpt = wpt; fpx = wx; fpy = wy; fpt = w_t;
                    if (ok) {
                        fsx = wx; fsy = wy; fst = w_t;
                        wx = wx - gam * (wx - opx); wy = wy - gam * (wy - opy); w_t = w_t - gam * (w_t - opt);
                    }
                    aa_hs = 1.0;
                    if (ok) { aa_normg = sqrt(rr[4]); aa_pending = true; w_changed = true; } else aa_iter = 0;
                } else {
                    xpx = wpx; xpy = wpy; xpt = wpt; fpx = wx; fpy = wy; fpt = w_t;
                    aa_hs = 1.0;
                }
                aa_iter++;
            }
            if (w_changed && !(check && iter > 0)) phiw = wave_sum(phix * wx + phiy * wy);      // (the renormalisation below recomputes phi . w itself)
        }
        if (check && iter > 0) {   // keep the homogeneous iterate in range
            const double nw = sqrt(wave_sum(fma(wx, wx, wy * wy)) + w_t * w_t);
            if (nw > 0) {
                const double f = sqrt((double)l) / nw;
                wx *= f; wy *= f; w_t *= f;
                if (aa_on) { aa_hs *= f; aa_normg *= f; }      // the map is positively homogeneous: the stored history scales with w (lazily)
            }
            phiw = wave_sum(phix * wx + phiy * wy);
        }
        if (aa_on && (aa_pending || (iter + 1) % aa_int == 0)) { aa_stale = false; wpx = wx; wpy = wy; wpt = w_t; }      // input of this iteration, where the next one needs it
        // S1 .. S5: p_x = G (rho_x w_x - A^T w_y), A p_x
        stage_y(yb, wy);
        wv_sync();
        const double tx = rho_x * wx - ATv(yb);
        stage_x(xb, tx);
        wv_sync();
        const double px = Gv(xb);
        stage_x(xb2, px);
        wv_sync();
        const double apx = Av(xb2);
        // S6/S7: tau-tilde, u-tilde, cone input
        const double tau_t = (rtau * w_t + phiw) / (rtau + hg);
        utx = px - tau_t * gx; ux = 2 * utx - wx;
        uty = (wy + dyl * apx) - tau_t * gy; uy = 2 * uty - wy;
        if (!ym) { uty = 0.0; uy = 0.0; }
        if (lane >= z && lane < zl && uy < 0) uy = 0;      // nonneg rows; zero-cone dual is free
        ut_t = tau_t; u_t = fmax(0.0, 2 * tau_t - w_t);
        // S8: second-order cones, one segment reduction each
        for_cones([&](int r0, int r1) {
            const double t0 = lane_bcast(uy, r0);
            if (r1 - r0 == 1) { if (lane == r0) uy = fmax(t0, 0.0); return; }
            const bool tail = lane > r0 && lane < r1;
            const double nz = sqrt(wave_sum(tail ? uy * uy : 0.0));
            double c0, f;
            if (nz <= t0) { c0 = t0; f = 1.0; }
            else if (nz <= -t0) { c0 = 0.0; f = 0.0; }
            else { c0 = 0.5 * (t0 + nz); f = c0 / nz; }
            if (lane == r0) uy = c0; else if (tail) uy = f * uy;
        });
        // ---- termination test / adaptive scale (wave-uniform branch)
        bool stop = false;
        if (check) {
            wv_sync();
            stage_x(xb, ux); stage_y(yb2, uy);
            wv_sync();
            const double ax0 = Av(xb), aty0 = ATv(yb2);      // A-hat x-hat ; A-hat^T y-hat
            tau = fabs(u_t);
            kap = fabs(rtau * (u_t + w_t - 2 * ut_t));
            const double isg = 1.0 / sigma;
            double r[8];   // rp, nax, ns, naxs, rd, naty (max) ; ctx, bty (sum)
            {
                const double sc = isg / Dv;
                const double ax = ax0 * sc, sh = (uy + wy - 2 * uty) / dyl * sc, bt = bv * tau * sc;
                r[0] = fabs(ax + sh - bt); r[1] = fabs(ax); r[2] = fabs(sh); r[3] = fabs(ax + sh);
                r[7] = bv * uy * isg * isg;
            }
            {
                const double sc = isg / Ev;
                const double aty = aty0 * sc;
                r[4] = fabs(aty + cv * tau * sc); r[5] = fabs(aty);
                r[6] = cv * ux * isg * isg;
            }
#pragma unroll
            for (int k = 0; k < 6; k++) r[k] = wv_max(r[k]);
            r[6] = wave_sum(r[6]); r[7] = wave_sum(r[7]);
            const double rp = r[0], nax = r[1], ns = r[2], naxs = r[3], rd = r[4], naty = r[5];
            ctx = r[6]; bty = r[7];
            if (tau > 0) {
                res_pri = rp / tau; res_dual = rd / tau; gap = fabs(ctx + bty) / tau;
                const double prl = fmax(fmax(nrm_b0 * tau, ns), nax) / tau, drl = fmax(nrm_c0 * tau, naty) / tau;
                const double grl = fmax(fabs(ctx), fabs(bty)) / tau;
                if (res_pri <= S.eps_abs + S.eps_rel * prl && res_dual <= S.eps_abs + S.eps_rel * drl &&
                    gap <= S.eps_abs + S.eps_rel * grl) { status = 1; stop = true; }
            }
            if (!stop && bty < 0 && naty / (-bty) <= S.eps_infeas) { status = -2; stop = true; }
            if (!stop && ctx < 0 && naxs / (-ctx) <= S.eps_infeas) { status = -1; stop = true; }
            if (!stop && S.adaptive_scale && iter > 0) {
                const double dp = fmax(fmax(nax, ns), nrm_b0 * tau), dd = fmax(naty, nrm_c0 * tau);
                const double rel_p = rp / (dp > 0 ? dp : 1), rel_d = rd / (dd > 0 ? dd : 1);
                if (rel_p > 0 && rel_d > 0 && isfinite(rel_p) && isfinite(rel_d)) {
                    sum_log += log(rel_p) - log(rel_d); n_log++;
                    const double factor = sqrt(exp(sum_log / n_log));
                    if (iter - last_scale_iter >= RESCALING_MIN_ITERS) {
                        const double ns2 = fmin(fmax(scale * factor, MIN_SCALE_VALUE), MAX_SCALE_VALUE);
                        if (ns2 != scale && (factor > sqrt(10.0) || factor < 1.0 / sqrt(10.0))) {
                            // keep (s, kappa):  R+ (w+ + u - 2 ut) = rsk  ->  w_y+ = rsk_y / r_y+ + 2 ut_y - u_y
                            const double dy_ratio = ns2 / scale;       // Dy+ / Dy, same for zero and cone rows
                            wy = (uy + wy - 2 * uty) * dy_ratio + 2 * uty - uy;
                            sum_log = 0; n_log = 0; last_scale_iter = iter; scale = ns2; aa_iter = 0; aa_pending = false; aa_stale = true;
                            refactor();
                            phiw = wave_sum(phix * wx + phiy * wy);
                        }
                    }
                }
            }
        }
        if (stop) break;
        if (iter + 1 >= S.max_iters) { iter++; break; }   // keep w pre-update so (s, kappa) match the last cone step
        // S9: relaxed update of w, and phi.w for the next iteration
        wx += alpha * (ux - utx); wy += alpha * (uy - uty); w_t += alpha * (u_t - ut_t);
        phiw = wave_sum(phix * wx + phiy * wy);
        wv_sync();      // (the staging buffers are rewritten at the top)
    }

    const double isg = 1.0 / sigma;
    if (status == 0) {   // ran out of iterations (SCS set_unfinished)
        tau = fabs(u_t);
        kap = fabs(rtau * (u_t + w_t - 2 * ut_t));
        const double r0 = wave_sum(cv * ux * isg * isg), r1 = wave_sum(bv * uy * isg * isg);
        if (tau > kap) status = 2; else if (r1 < r0) status = -7; else status = -6;
    }
    // ---------------------------------------------------------------- write back (un-normalise)
    {
        const bool solved = (status == 1 || status == 2);
        const bool infeas = (status == -2 || status == -7);
        const double it = solved ? 1.0 / (sigma * tau) : isg;
        if (xm) xo[inst * n + lane] = infeas ? NAN : Ev * ux * it;
        if (ym) {
            const double sh = (uy + wy - 2 * uty) / dyl;
            yo[inst * m + lane] = (solved || infeas) ? Dv * uy * it : NAN;
            so[inst * m + lane] = infeas ? NAN : sh / Dv * it;
        }
        if (lane == 0) {
            iters_o[inst] = iter; status_o[inst] = status;
            if (resid_o) { resid_o[3 * inst] = res_pri; resid_o[3 * inst + 1] = res_dual; resid_o[3 * inst + 2] = gap; }
        }
    }
}

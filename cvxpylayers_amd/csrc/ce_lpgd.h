// ce_lpgd.h -- Lagrangian proximal gradient descent (LPGD) backward: the data of a perturbed program and the differenced envelope gradients of two of its
// solutions (cone_engine.hip ce_lpgd_perturb, ce_lpgd_grad; tests/test_gpu_lpgd_kernels.py)
//
//   perturbed program at +tau:  c+ = c + tau dx - rho x*,  b+ = b - tau dy,  P+ = P + rho I,  A unchanged        (cotangents dx on x*, dy on y*)
//   gradient:  dtheta = [G(x_b, y_b) - G(x_a, y_a)] / delta    with G = dL/dtheta, the envelope gradients of ce_value.h:
//   G_A[k] = -y_row x_col (A entry) / -y_row (b entry) in the boundary convention A_eval = [-A.data, b],  G_q = [x; 0],  G_P[k] = w x_r x_c
// Every product difference is formed from the differences of the points, never from two large products:
//   y_b,r x_b,c - y_a,r x_a,c = y_b,r Dx_c + Dy_r x_a,c        (Dx = x_b - x_a, Dy = y_b - y_a; the same for x_r x_c)
// Not a tiled family: no row in ce_variants.h.  Plain C++, vector stores.  Thread count, instances per workgroup, tile and LDS pitch are ce_value.h's.
#pragma once
#include "ce_value.h"

// One workgroup = VAL_IPB instances, lanes over the entries (the structure's row / column of an entry is fetched once for all of them).  Writes
//   q_out = fma(-rho, x*, fma(tau, dx, q)) on the first n rows, q's last row (the constant d) unchanged, under q's own stride pair;
//   A_out (batch-major rows nnz_aug apart), when dy is given: a copy of A whose b entries -- column n of the structure -- moved by -tau dy[row];
//   P_out = P + rho on the diagonal entries, when the host asks for it (a P structure and rho != 0);
//   flags[i]: bit 0 = every entry of dx and dy of the instance is exactly zero, bit 1 = some dy[r] != 0 sits on a row without a b entry (bpos[r] < 0: dropped).
__global__ void __launch_bounds__(VAL_NT) k_lpgd_perturb(CeLpgdPerturbArgs a) {
    const int n = a.n, m = a.m, t = threadIdx.x, i0 = blockIdx.x * VAL_IPB, nu = min(VAL_IPB, a.B - i0);
    for (int u = 0; u < nu; u++) {          // (nu is uniform over the workgroup: every thread reaches the votes)
        const size_t i = (size_t)i0 + u;
        int nz = 0, drop = 0;
        for (int j = t; j < n; j += VAL_NT) nz |= a.dx[i * n + j] != 0.0;
        if (a.dy)
            for (int r = t; r < m; r += VAL_NT) { const int v = a.dy[i * m + r] != 0.0; nz |= v; drop |= v && a.bpos[r] < 0; }
        nz = __syncthreads_or(nz); drop = __syncthreads_or(drop);
        if (t == 0) a.flags[i] = (nz ? 0 : 1) | (drop ? 2 : 0);
    }
    for (int j = t; j <= n; j += VAL_NT)
        for (int u = 0; u < nu; u++) {
            const size_t i = (size_t)i0 + u;
            const long at = j * a.sqk + (long)i * a.sqb;
            double v = a.q[at];
            if (j < n) {
                v = fma(a.tau, a.dx[i * n + j], v);
                if (a.rho != 0.0) v = fma(-a.rho, a.x[i * n + j], v);
            }
            a.q_out[at] = v;
        }
    if (a.dy && a.A_out)
        for (int k = t; k < a.nnz_aug; k += VAL_NT) {
            const int r = a.rowidx[k], c = a.colidx[k];
            for (int u = 0; u < nu; u++) {
                const size_t i = (size_t)i0 + u;
                double v = a.A[i * a.sAb + k];
                if (c >= n) v = fma(-a.tau, a.dy[i * m + r], v);
                a.A_out[i * a.nnz_aug + k] = v;
            }
        }
    if (a.P_out)
        for (int k = t; k < a.nnz_p; k += VAL_NT) {
            const double add = a.prow[k] == a.pcol[k] ? a.rho : 0.0;
            for (int u = 0; u < nu; u++) { const size_t at = ((size_t)i0 + u) * a.nnz_p + k; a.P_out[at] = a.P[at] + add; }
        }
}

// what both gradient kernels stage per instance: x_a, x_b, Dx / delta, -y_b, -Dy / delta (the signs of G_A folded in, the scaling applied once).  An instance
// with skip[i] != 0 stages exact zeros whatever its inputs hold (selects in front of the arithmetic: NaN never enters a difference or a product).
struct LpgdX { double xa, xb, dx; };
struct LpgdY { double nyb, ndy; };
__device__ inline LpgdX lpgd_stage_x(const CeLpgdGradArgs &a, bool on, size_t at) {
    const double xa = on ? a.xa[at] : 0.0, xb = on ? a.xb[at] : 0.0;
    return {xa, xb, (xb - xa) / a.delta};
}
__device__ inline LpgdY lpgd_stage_y(const CeLpgdGradArgs &a, bool on, size_t at) {
    const double ya = on ? a.ya[at] : 0.0, yb = on ? a.yb[at] : 0.0;
    return {-yb, (ya - yb) / a.delta};
}
// entry k of dA from the staged values: (row r, column c < n) -(y_b,r Dx_c + Dy_r x_a,c) / delta, (row r, column n: a b entry) -Dy_r / delta
__device__ inline double lpgd_dA(bool is_A, double nyb_r, double ndy_r, double dx_c, double xa_c) { return is_A ? fma(ndy_r, xa_c, nyb_r * dx_c) : ndy_r; }

// BATCH-MAJOR rows (sdAk == 1): the layout of k_value_vjp_rows.  Also writes dq (any stride pair) and the batch-major dP.
__global__ void __launch_bounds__(VAL_NT) k_lpgd_grad_rows(CeLpgdGradArgs a) {
    extern __shared__ double lpgd_lds[];
    const int n = a.n, m = a.m, t = threadIdx.x, i0 = blockIdx.x * VAL_IPB;
    double *xas = lpgd_lds, *xbs = xas + VAL_IPB * n, *dxs = xbs + VAL_IPB * n, *nyb = dxs + VAL_IPB * n, *ndy = nyb + VAL_IPB * m;
    for (int u = 0; u < VAL_IPB; u++) {
        const int i = i0 + u;
        const bool on = i < a.B && !(a.skip && a.skip[i]);
        for (int j = t; j < n; j += VAL_NT) { const LpgdX v = lpgd_stage_x(a, on, (size_t)i * n + j); xas[u * n + j] = v.xa; xbs[u * n + j] = v.xb; dxs[u * n + j] = v.dx; }
        for (int r = t; r < m; r += VAL_NT) { const LpgdY v = lpgd_stage_y(a, on, (size_t)i * m + r); nyb[u * m + r] = v.nyb; ndy[u * m + r] = v.ndy; }
    }
    const bool tri = a.dP && a.nnz_p > 0 && val_one_triangle(a.prow, a.pcol, a.nnz_p);
    __syncthreads();
    const int nu = min(VAL_IPB, a.B - i0);
    if (a.dA && a.sdAk == 1)
        for (int k = t; k < a.nnz_aug; k += VAL_NT) {
            const int r = a.rowidx[k], c = a.colidx[k];
            const bool is_A = c < n;
            for (int u = 0; u < nu; u++)
                a.dA[(size_t)(i0 + u) * a.sdAb + k] = lpgd_dA(is_A, nyb[u * m + r], ndy[u * m + r], is_A ? dxs[u * n + c] : 0.0, is_A ? xas[u * n + c] : 0.0);
        }
    if (a.dq)
        for (int j = t; j <= n; j += VAL_NT)
            for (int u = 0; u < nu; u++) a.dq[j * a.sdqk + (i0 + u) * a.sdqb] = j < n ? dxs[u * n + j] : 0.0;
    if (a.dP)
        for (int k = t; k < a.nnz_p; k += VAL_NT) {
            const int r = a.prow[k], c = a.pcol[k];
            const bool in = (unsigned)r < (unsigned)n && (unsigned)c < (unsigned)n;
            const double w = (tri && r != c) ? 1.0 : 0.5;
            for (int u = 0; u < nu; u++)
                a.dP[(size_t)(i0 + u) * a.nnz_p + k] = in ? w * fma(dxs[u * n + r], xas[u * n + c], xbs[u * n + r] * dxs[u * n + c]) : 0.0;
        }
}

// dA in the BATCH-MINOR layout (sdAb == 1): the tile of k_value_vjp_tile -- 64 instances, lanes over the instances, workgroup (tile, chunk) serves the entries
// [chunk * kchunk, (chunk + 1) * kchunk), chunk 0 also writes dq when told to (wdq: sdqb == 1).  STAGED: the tile's staged values sit in LDS, instance-minor with
// pitch VAL_TLD; otherwise -- templates whose tile exceeds LDS -- the lanes gather the points from global memory (L2) and difference them per entry.
template <bool STAGED>
__global__ void __launch_bounds__(VAL_NT) k_lpgd_grad_tile(CeLpgdGradArgs a, int kchunk, int wdq) {
    extern __shared__ double lpgd_lds[];
    const int n = a.n, m = a.m, t = threadIdx.x, i0 = blockIdx.x * VAL_TI;
    const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), nw = VAL_NT / 64;
    const int i = i0 + lane;
    const bool on = i < a.B && !(a.skip && a.skip[i]);
    double *xas = lpgd_lds, *dxs = xas + (size_t)n * VAL_TLD, *nyb = dxs + (size_t)n * VAL_TLD, *ndy = nyb + (size_t)m * VAL_TLD;
    if (STAGED) {
        // the tile's rows of x (and of y) are one contiguous range: coalesced reads, transposing LDS writes
        const int ni = min(VAL_TI, a.B - i0);
        for (int f = t; f < VAL_TI * n; f += VAL_NT) {
            const int u = f / n, j = f - u * n;
            const LpgdX v = lpgd_stage_x(a, u < ni && !(a.skip && a.skip[i0 + u]), (size_t)i0 * n + f);
            xas[j * VAL_TLD + u] = v.xa; dxs[j * VAL_TLD + u] = v.dx;
        }
        for (int f = t; f < VAL_TI * m; f += VAL_NT) {
            const int u = f / m, r = f - u * m;
            const LpgdY v = lpgd_stage_y(a, u < ni && !(a.skip && a.skip[i0 + u]), (size_t)i0 * m + f);
            nyb[r * VAL_TLD + u] = v.nyb; ndy[r * VAL_TLD + u] = v.ndy;
        }
        __syncthreads();
    }
    const int k0 = blockIdx.y * kchunk, k1 = min(a.nnz_aug, k0 + kchunk);
    if (a.dA)
        for (int k = k0 + wave; k < k1; k += nw) {
            const int r = a.rowidx[k], c = a.colidx[k];
            const bool is_A = c < n;
            double v;
            if (STAGED) v = lpgd_dA(is_A, nyb[r * VAL_TLD + lane], ndy[r * VAL_TLD + lane], is_A ? dxs[c * VAL_TLD + lane] : 0.0, is_A ? xas[c * VAL_TLD + lane] : 0.0);
            else {
                const LpgdY y = lpgd_stage_y(a, on, (size_t)i * m + r);
                const LpgdX x = lpgd_stage_x(a, on && is_A, (size_t)i * n + (is_A ? c : 0));
                v = lpgd_dA(is_A, y.nyb, y.ndy, x.dx, x.xa);
            }
            if (i < a.B) a.dA[k * a.sdAk + i * a.sdAb] = v;
        }
    if (wdq && blockIdx.y == 0 && i < a.B)
        for (int j = wave; j <= n; j += nw) {
            double v = 0.0;
            if (j < n) v = STAGED ? dxs[j * VAL_TLD + lane] : lpgd_stage_x(a, on, (size_t)i * n + j).dx;
            a.dq[j * a.sdqk + i * a.sdqb] = v;
        }
}

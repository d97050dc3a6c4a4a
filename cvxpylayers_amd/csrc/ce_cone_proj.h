// ce_cone_proj.h -- the Euclidean projection onto a product of cones and its derivative as kernels of their own (ce_cone_project / ce_cone_dproject):
// v (B, m) -> Pi_K(v) or Pi_K*(v), and dir -> D Pi(v) dir.  Included inside an anonymous namespace.
//
// The work per item differs by orders of magnitude between a clipped row and an eigendecomposition, so the decomposition is by cone KIND, one launch per kind
// present and none for a kind that is absent:
//   k_cone_rows<DPROJ>  zero / nonnegative rows (one lane per row) and second-order cones (a 16-lane row per cone of dimension <= 16, four to a wave; a wave per
//                       larger cone).  No LDS, no barrier: the ||z|| and z . dz reductions are DPP butterflies inside the wave.  Memory bound (16 B per row
//                       for Pi, 24 B for D Pi).  The three lane shapes are segments of ONE grid (a workgroup is of one shape).
//   k_cone_psd          one workgroup per (instance, block): psd_project_mfma cold (orders <= 39, matrix cores) or psd_project (psd_jacobi, plain FMA); with
//                       `state` the eigenvectors and the unclipped eigenvalues are kept.
//   k_cone_dpsd         V (B o (V^T H V)) V^T from that state, four k x k x k contractions: psd_mfma_gemm (v_mfma_f64_16x16x4_f64) up to order 39, plain FMA above.
//   k_cone_triples      one thread per (instance, triple): cone_triple_project (ce_cone_proj_triple.h) from a cold root, its Jacobian to `state`.
//   k_cone_dtriples     a 3 x 3 product from `state`.
// The derivative is symmetric for every kind, so D Pi(v) dir serves both the forward and the reverse mode.
//
// Conventions at kinks (oracle/cone_oracle.c dproj_dual_cone, dproj_soc, dproj_psd): a nonnegative row at exactly 0 has the factor 1/2; a second-order cone
// follows ns_soc_kind (inclusive boundaries: the identity on the cone's boundary, 0 on the polar's); the divided differences of a PSD block are 1 for two
// positive eigenvalues, 0 for two non-positive ones, (p_i - p_j) / (w_i - w_j) otherwise; triples: what exp_dproject / pow_dproject return.
// A non-finite entry turns the rows of the cone that holds it into NaN and leaves every other cone alone.
//
// Trip bounds (every loop is bounded by the cone set alone, never by the data): the strided passes over a cone's rows (<= d / 64 + 1, k^2 / 256 + 1); psd_sweeps_wg
// and psd_jacobi 40 sweeps of k - 1 rounds; the contractions k (or ceil(k / 4) matrix-core steps); exp_project / pow_project 120 Newton steps, the 3 x 3
// and 4 x 4 eliminations of their Jacobians fixed.
#pragma once
#include "ce_common.h"
#include "ce_backward_ns.h"         // ns_soc_kind: the one statement of the second-order cone's three cases
#include "ce_psd_jacobi.h"          // psd_project
#include "ce_psd_mfma.h"            // psd_project_mfma, psd_mfma_gemm
#include "ce_cone_proj_triple.h"    // cone_triple_project
#include "ce_cone_proj_types.h"

static_assert(CONE_PROJ_NT == NT, "the PSD routines reduce over NT threads");

__device__ __forceinline__ bool cone_finite(double w) { return fabs(w) < INFINITY; }

// instance and position inside it of flat item `idx` of B * per items (32-bit division whenever the count allows it)
__device__ __forceinline__ void cone_split(long long idx, long long total, int per, long long &inst, int &pos) {
    if ((total >> 32) == 0) { const unsigned u = (unsigned)idx, qd = u / (unsigned)per; inst = qd; pos = (int)(u - qd * (unsigned)per); }
    else { inst = idx / per; pos = (int)(idx - inst * per); }
}

// one second-order cone held by a group of lanes: every lane has the cone's t (t0) and the squared norm of z (nz2); `each(f)` visits the lane's own z rows
// as f(row, z_row, dir_row) and `sum` adds over the group.  DPROJ: gt = dir's t row.
template <bool DPROJ, class Each, class Sum, class Put>
__device__ __forceinline__ void cone_soc(int d, double t0, double nz2, double gt, bool lead, Each &&each, Sum &&sum, Put &&put) {
    const double nz = sqrt(nz2);
    double lam;
    const int kind = ns_soc_kind(d, t0, nz, lam);
    const bool bad = !cone_finite(t0) || !cone_finite(nz2);
    if constexpr (!DPROJ) {
        if (bad) lam = NAN; else if (kind == 0) lam = 1.0;          // Pi(v) = v inside the cone, 0 inside the polar, lam (||z||, z) between
        each([&](int i, double zi, double) { put(i, lam * zi); });
        if (lead) put(0, (kind == 2 || bad) ? lam * nz : lam * t0);
    } else {
        double zg = 0.0;
        each([&](int, double zi, double gi) { zg = fma(zi, gi, zg); });
        zg = sum(zg);
        // kind 2:  d t = (g_t + u) / 2,  d z = lam g_z + (g_t - t u / ||z||) / (2 ||z||) z,   u = z . g_z / ||z||
        const double u = zg / nz, ct = 0.5 * (gt - t0 * u / nz) / nz;
        const double f = bad ? NAN : (kind == 0 ? 1.0 : (kind == 1 ? 0.0 : lam)), cz = (kind == 2 && !bad) ? ct : 0.0;
        each([&](int i, double zi, double gi) { put(i, fma(cz, zi, f * gi)); });
        if (lead) put(0, (kind == 2 && !bad) ? 0.5 * (gt + u) : f * gt);
    }
}

// grid: nb_plain workgroups of rows, then nb_small of 16-lane cones, then the wave-per-cone ones
template <bool DPROJ>
__global__ void __launch_bounds__(CONE_PROJ_NT)
k_cone_rows(ConeProjArgs a, int nb_plain, int nb_small) {
    const ConeProjDev &D = a.D;
    const int tid = threadIdx.x, blk = blockIdx.x;
    if (blk < nb_plain) {
        const int zl = D.z + D.l;
        const long long total = (long long)a.B * zl, idx = (long long)blk * CONE_PROJ_NT + tid;
        if (idx >= total) return;
        long long inst; int i;
        cone_split(idx, total, zl, inst, i);
        const double w = a.v[inst * a.ldv + i];
        const bool zrow = i < D.z;
        double r;
        if constexpr (!DPROJ) {
            if (zrow) r = a.dual ? w : w - w;                        // zero cone: 0 (NaN stays NaN); its dual is free
            else r = w < 0 ? 0.0 : w;
        } else {
            const double g = a.dir[inst * a.lddir + i];
            if (zrow) r = a.dual ? g : 0.0;
            else r = w > 0 ? g : (w < 0 ? 0.0 : (w == 0 ? 0.5 * g : NAN));
        }
        a.out[inst * a.ldout + i] = r;
    } else if (blk < nb_plain + nb_small) {
        // every lane of the wave stays active: the butterflies of group_reduce read their neighbours
        const long long total = (long long)a.B * D.nq_small, g = ((long long)(blk - nb_plain) * CONE_PROJ_NT + tid) >> 4;
        const int l16 = tid & 15;
        const bool cv = g < total;
        long long inst; int ci;
        cone_split(cv ? g : 0, total, D.nq_small, inst, ci);
        const int c = D.soc_small[ci], r0 = D.qoff[c], d = D.qoff[c + 1] - r0;
        const double *vp = a.v + inst * a.ldv + r0;
        const double *gp = DPROJ ? a.dir + inst * a.lddir + r0 : vp;
        double *op = a.out + inst * a.ldout + r0;
        const bool mine = cv && l16 > 0 && l16 < d;
        const double t0 = vp[0], zi = mine ? vp[l16] : 0.0, gi = (DPROJ && mine) ? gp[l16] : 0.0, gt = DPROJ ? gp[0] : 0.0;
        const double nz2 = group_reduce<16, false>(zi * zi);
        cone_soc<DPROJ>(d, t0, nz2, gt, cv && l16 == 0,
                        [&](auto &&f) { if (mine) f(l16, zi, gi); },
                        [&](double s) { return group_reduce<16, false>(s); },
                        [&](int i, double r) { op[i] = r; });
    } else {
        const long long total = (long long)a.B * D.nq_large, wv = ((long long)(blk - nb_plain - nb_small) * CONE_PROJ_NT + tid) >> 6;
        const int lane = tid & 63;
        if (wv >= total) return;                                    // (a whole wave)
        long long inst; int ci;
        cone_split(wv, total, D.nq_large, inst, ci);
        const int c = D.soc_large[ci], r0 = D.qoff[c], d = D.qoff[c + 1] - r0;
        const double *vp = a.v + inst * a.ldv + r0;
        const double *gp = DPROJ ? a.dir + inst * a.lddir + r0 : vp;
        double *op = a.out + inst * a.ldout + r0;
        double nz2 = 0.0;
        for (int i = 1 + lane; i < d; i += 64) { const double w = vp[i]; nz2 = fma(w, w, nz2); }
        nz2 = wave_sum(nz2);
        cone_soc<DPROJ>(d, vp[0], nz2, DPROJ ? gp[0] : 0.0, lane == 0,
                        [&](auto &&f) { for (int i = 1 + lane; i < d; i += 64) f(i, vp[i], DPROJ ? gp[i] : 0.0); },      // (second pass: the rows come from the cache)
                        [&](double s) { return wave_sum(s); },
                        [&](int i, double r) { op[i] = r; });
    }
}

// ---- PSD blocks ---------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CONE_PROJ_NT)
k_cone_psd(ConeProjArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const ConeProjDev &D = a.D;
    const int inst = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    const int k = D.sord[c], nsv = k * (k + 1) / 2;
    const double *vs = a.v + (size_t)inst * a.ldv + D.soff[c];
    double *os = a.out + (size_t)inst * a.ldout + D.soff[c];
    double *st = a.state ? a.state + (size_t)inst * D.state_len + D.sstate[c] : nullptr;
    int bad = 0;
    for (int pos = tid; pos < nsv; pos += CONE_PROJ_NT) { const double w = vs[pos]; os[pos] = w; bad |= !cone_finite(w); }
    // workgroup vote through the dynamic LDS (no static LDS in front of it: the footprint of ce_lds_cone_proj.h is all the kernel holds)
    if ((tid & 63) == 0) sm[tid >> 6] = 0.0;
    __syncthreads();
    if (bad) sm[tid >> 6] = 1.0;
    __syncthreads();
    bad = 0;
    for (int w = 0; w < CONE_PROJ_NT / 64; w++) bad |= sm[w] != 0.0;
    __syncthreads();
    if (bad) {                                                      // uniform: no sweep runs on a non-finite block
        for (int pos = tid; pos < nsv; pos += CONE_PROJ_NT) os[pos] = NAN;
        if (st) for (int idx = tid; idx < k * k + k; idx += CONE_PROJ_NT) st[idx] = NAN;
        return;
    }
    const int R = cone_proj_psd_rows(k), P = cone_proj_psd_pitch(k);
    double *Sm = sm, *Vm = Sm + R * P, *Tm = Vm + R * P, *cs = Tm + R * P, *red = cs + 3 * R + 16;
    if (k <= CONE_PROJ_PSD_MFMA_MAX) {
        psd_project_mfma<CONE_PROJ_NT>(os, k, Sm, Vm, Tm, cs, red, st, 0);        // cold; the eigenvectors go to st[0 .. k^2)
        if (st) for (int i = tid; i < k; i += CONE_PROJ_NT) st[k * k + i] = Sm[i * P + i];
    } else {
        psd_project<CONE_PROJ_NT>(os, k, Sm, Vm, cs, red);
        if (st) {
            for (int idx = tid; idx < k * k; idx += CONE_PROJ_NT) st[idx] = Vm[idx];
            for (int i = tid; i < k; i += CONE_PROJ_NT) st[k * k + i] = Sm[i * k + i];
        }
    }
}

// out(M, N, sum_K fa(M, K) fb(K, N)) on a k x k block: the matrix cores on zero-padded KP x KP storage, or one thread per entry
template <bool MFMA, class FA, class FB, class FO>
__device__ __forceinline__ void cone_contract(int k, FA &&fa, FB &&fb, FO &&out) {
    if constexpr (MFMA) psd_mfma_gemm<CONE_PROJ_NT>(psd_mfma_kp(k) / 16, fa, fb, out, (k + 3) >> 2);
    else {
        for (int idx = threadIdx.x; idx < k * k; idx += CONE_PROJ_NT) {
            const int i = idx / k, j = idx - i * k;
            double a0 = 0.0, a1 = 0.0;
            int e = 0;
            for (; e + 1 < k; e += 2) { a0 = fma(fa(i, e), fb(e, j), a0); a1 = fma(fa(i, e + 1), fb(e + 1, j), a1); }
            if (e < k) a0 = fma(fa(i, e), fb(e, j), a0);
            out(i, j, a0 + a1);
        }
    }
}

// divided difference of p = max(w, 0) between two eigenvalues
__device__ __forceinline__ double cone_psd_divdiff(double wi, double wj) {
    if (wi > 0 && wj > 0) return 1.0;
    if (!(wi > 0) && !(wj > 0)) return (wi != wi || wj != wj) ? NAN : 0.0;
    return (fmax(wi, 0.0) - fmax(wj, 0.0)) / (wi - wj);
}

template <bool MFMA>
__device__ __forceinline__ void cone_dpsd_block(int k, const double *st, const double *ds, double *os, double *sm) {
    const int tid = threadIdx.x;
    const int R = cone_proj_psd_rows(k), P = cone_proj_psd_pitch(k);
    double *Hm = sm, *Vm = Hm + R * P, *Tm = Vm + R * P, *w = Tm + R * P;
    for (int idx = tid; idx < R * R; idx += CONE_PROJ_NT) {
        const int i = idx / R, j = idx - i * R;
        double hv = 0.0, vv = 0.0;
        if (i < k && j < k) {
            const int r = i >= j ? i : j, cl = i >= j ? j : i;      // lower-triangle entry (r, cl), column-major packed
            const double x = ds[cl * k - (cl * (cl - 1)) / 2 + (r - cl)];
            hv = (r == cl) ? x : x * M_SQRT1_2;
            vv = st[i * k + j];
        }
        Hm[i * P + j] = hv; Vm[i * P + j] = vv;
    }
    for (int i = tid; i < R; i += CONE_PROJ_NT) w[i] = i < k ? st[k * k + i] : 0.0;
    __syncthreads();
    cone_contract<MFMA>(k, [&](int M, int K) { return Hm[K * P + M]; }, [&](int K, int N) { return Vm[K * P + N]; },        // T = H V (H symmetric: read along rows)
                        [&](int M, int N, double x) { Tm[M * P + N] = x; });
    __syncthreads();
    cone_contract<MFMA>(k, [&](int M, int K) { return Vm[K * P + M]; }, [&](int K, int N) { return Tm[K * P + N]; },        // H <- B o (V^T T)
                        [&](int M, int N, double x) { Hm[M * P + N] = x * cone_psd_divdiff(w[M], w[N]); });
    __syncthreads();
    cone_contract<MFMA>(k, [&](int M, int K) { return Vm[M * P + K]; }, [&](int K, int N) { return Hm[K * P + N]; },        // T = V H
                        [&](int M, int N, double x) { Tm[M * P + N] = x; });
    __syncthreads();
    cone_contract<MFMA>(k, [&](int M, int K) { return Tm[M * P + K]; }, [&](int K, int N) { return Vm[N * P + K]; },        // H <- T V^T
                        [&](int M, int N, double x) { Hm[M * P + N] = x; });
    __syncthreads();
    for (int idx = tid; idx < k * k; idx += CONE_PROJ_NT) {
        const int r = idx / k, cl = idx - r * k;
        if (r < cl) continue;
        const double x = 0.5 * (Hm[r * P + cl] + Hm[cl * P + r]);
        os[cl * k - (cl * (cl - 1)) / 2 + (r - cl)] = (r == cl) ? x : x * M_SQRT2;
    }
}

__global__ void __launch_bounds__(CONE_PROJ_NT)
k_cone_dpsd(ConeProjArgs a) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const ConeProjDev &D = a.D;
    const int inst = blockIdx.x, c = blockIdx.y;
    const int k = D.sord[c];
    const double *st = a.state + (size_t)inst * D.state_len + D.sstate[c];
    const double *ds = a.dir + (size_t)inst * a.lddir + D.soff[c];
    double *os = a.out + (size_t)inst * a.ldout + D.soff[c];
    if (k <= CONE_PROJ_PSD_MFMA_MAX) cone_dpsd_block<true>(k, st, ds, os, sm);      // (uniform)
    else cone_dpsd_block<false>(k, st, ds, os, sm);
}

// ---- exponential / power triples ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CONE_PROJ_NT)
k_cone_triples(ConeProjArgs a) {
    const ConeProjDev &D = a.D;
    const int ntri = D.nep + D.np;
    const long long total = (long long)a.B * ntri, idx = (long long)blockIdx.x * CONE_PROJ_NT + threadIdx.x;
    if (idx >= total) return;
    long long inst; int c;
    cone_split(idx, total, ntri, inst, c);
    const double *vp = a.v + inst * a.ldv + D.e_row0 + 3 * c;
    const double vv[3] = {vp[0], vp[1], vp[2]};
    double o[3], J[9];
    const bool is_exp = c < D.nep;
    cone_triple_project(vv, is_exp, is_exp ? 0.0 : D.pw[c - D.nep], a.dual, o, a.state ? J : nullptr);
    double *op = a.out + inst * a.ldout + D.e_row0 + 3 * c;
    op[0] = o[0]; op[1] = o[1]; op[2] = o[2];
    if (a.state) {
        double *st = a.state + inst * D.state_len + D.tri_state0 + 9 * c;
#pragma unroll
        for (int i = 0; i < 9; i++) st[i] = J[i];
    }
}

__global__ void __launch_bounds__(CONE_PROJ_NT)
k_cone_dtriples(ConeProjArgs a) {
    const ConeProjDev &D = a.D;
    const int ntri = D.nep + D.np;
    const long long total = (long long)a.B * ntri, idx = (long long)blockIdx.x * CONE_PROJ_NT + threadIdx.x;
    if (idx >= total) return;
    long long inst; int c;
    cone_split(idx, total, ntri, inst, c);
    const double *st = a.state + inst * D.state_len + D.tri_state0 + 9 * c;
    const double *gp = a.dir + inst * a.lddir + D.e_row0 + 3 * c;
    double *op = a.out + inst * a.ldout + D.e_row0 + 3 * c;
    const double g0 = gp[0], g1 = gp[1], g2 = gp[2];
#pragma unroll
    for (int i = 0; i < 3; i++) op[i] = fma(st[3 * i + 2], g2, fma(st[3 * i + 1], g1, st[3 * i] * g0));
}

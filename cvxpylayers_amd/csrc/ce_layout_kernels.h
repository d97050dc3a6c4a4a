// ce_layout_kernels.h -- the layout pass (k_transpose) and the parameter-map products (k_parammap*) the host launches itself (cone_engine.hip; tests/test_gpu_layout_kernels.py)
#pragma once
#include "ce_dA_entry.h"       // ce_dA_entry: the entry of the dA row, shared with k_backward_ns

// ================================================================================================
// layout kernels: (R x C) row-major <-> (C x R) row-major, fp64, 32x32 LDS tiles (+1 pad)
// ================================================================================================
// TS x TS tiles.  TS = 64 (the default of the launch sites, CE_TR_TILE): a wave reads and writes whole 512-byte row segments (with 32 a wave touches two 256-byte pieces of
// different rows) and every thread keeps 16 independent loads in flight before the barrier.
template <int TS>
__global__ void __launch_bounds__(256) k_transpose(const double *__restrict__ in, double *__restrict__ out, int R, int C) {
    __shared__ double tile[TS][TS + 1];
    constexpr int RS = 256 / TS;          // rows of the tile per pass
    const int bx = blockIdx.x * TS, by = blockIdx.y * TS;
    const int tx = threadIdx.x % TS, ty = threadIdx.x / TS;
    double v[TS / RS];
#pragma unroll
    for (int u = 0; u < TS / RS; u++) { const int rr = by + ty + RS * u, cc = bx + tx; v[u] = (rr < R && cc < C) ? in[(size_t)rr * C + cc] : 0.0; }
#pragma unroll
    for (int u = 0; u < TS / RS; u++) tile[ty + RS * u][tx] = v[u];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < TS / RS; u++) { const int cc = bx + ty + RS * u, rr = by + tx; if (rr < R && cc < C) out[(size_t)cc * R + rr] = tile[tx][ty + RS * u]; }
}


// ================================================================================================
// k_expand_dA: the adjoint's dA, batch-minor (nnz_aug x B), written ONCE from the factor vectors of k_backward_ns's factor mode (cone_engine.hip ce_vjp_qp)
// ================================================================================================
// Entry k = (i, j) of instance b is  -(x_j v_i - y_i r_j)  (j < n)  or  -v_i  (the b column), with x, y the forward's outputs (batch-major), r = -dq (the adjoint's
// dq, entry j of instance b at j * sdqk + b * sdqb) and v = r_y, which the adjoint left in the first m doubles of the instance's row of `vf` (pitch ldv).  The
// batch-major row, a read of it and a batch-minor write of it (k_transpose) become this one store stream plus the factor reads.
//   grid.x: tiles of EXP_TB consecutive instances; grid.y: slabs of `slab` consecutive entries.  The workgroup stages the tile's x, y and v through LDS so that
//   lanes index instances (pitch EXP_TB + 1: the staging writes walk the rows) and the slab's (i, j) pairs once, packed; r is read where it lies, coalesced
//   along the batch.  A half-wave takes a contiguous run of the slab: consecutive entries of the value order mostly share their column, so x_j and r_j stay in
//   registers until j changes.  32 lanes store 32 consecutive instances of one entry: whole 64-byte lines when B is a multiple of 8.
//   adj[b] & 8: the LSQR re-solve behind the adjoint overwrote the WHOLE batch-major row of instance b (and its v with it): that lane copies its row instead
//   (a transposing read; such instances are rare).
constexpr int EXP_TB = 32, EXP_NT = 256, EXP_U = 4, EXP_SU = 8;
constexpr size_t EXPAND_LDS_MAX = 80 * 1024;          // two workgroups per CU; the host sets it as the kernel's dynamic-LDS limit (ce_create) and plans within it
inline size_t expand_dA_lds_bytes(int n, int m, int slab) { return sizeof(double) * (size_t)(n + 2 * m) * (EXP_TB + 1) + sizeof(int) * (size_t)slab; }
__global__ void __launch_bounds__(EXP_NT) k_expand_dA(int n, int m, int K, int B, int slab, const int *__restrict__ rowidx, const int *__restrict__ colidx,
                                                     const double *__restrict__ xg, const double *__restrict__ yg, const double *__restrict__ vf, long ldv,
                                                     const double *__restrict__ dq, long sdqk, long sdqb, const int *__restrict__ adj, double *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) double esm[];
    constexpr int P = EXP_TB + 1, NSUB = EXP_NT / EXP_TB;
    double *xs = esm, *ys = xs + (size_t)n * P, *vs = ys + (size_t)m * P;
    int *ij = (int *)(vs + (size_t)m * P);
    const int tid = threadIdx.x, bl = tid % EXP_TB, sub = tid / EXP_TB;
    const int b0 = blockIdx.x * EXP_TB, nb = min(EXP_TB, B - b0);
    const int k0 = blockIdx.y * slab, k1 = min(K, k0 + slab);
    // the tile's rows of x and of y are one contiguous run each; v is the head of every instance's row of vf
    // (EXP_SU loads in flight per thread in front of the LDS writes: one load per round trip would make the staging the longer half of the kernel)
    for (int i0 = tid; i0 < nb * n; i0 += EXP_SU * EXP_NT) {
        double t[EXP_SU];
#pragma unroll
        for (int u = 0; u < EXP_SU; u++) { const int idx = i0 + u * EXP_NT; t[u] = idx < nb * n ? xg[(size_t)b0 * n + idx] : 0.0; }
#pragma unroll
        for (int u = 0; u < EXP_SU; u++) { const int idx = i0 + u * EXP_NT, b = idx / n, j = idx - b * n; if (idx < nb * n) xs[j * P + b] = t[u]; }
    }
    for (int i0 = tid; i0 < nb * m; i0 += EXP_SU * EXP_NT) {
        double t[EXP_SU], w[EXP_SU];
#pragma unroll
        for (int u = 0; u < EXP_SU; u++) {
            const int idx = i0 + u * EXP_NT, b = idx / m, i = idx - b * m; const bool on = idx < nb * m;
            t[u] = on ? yg[(size_t)b0 * m + idx] : 0.0; w[u] = on ? vf[(size_t)(b0 + b) * ldv + i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < EXP_SU; u++) { const int idx = i0 + u * EXP_NT, b = idx / m, i = idx - b * m; if (idx < nb * m) { ys[i * P + b] = t[u]; vs[i * P + b] = w[u]; } }
    }
    for (int k = k0 + tid; k < k1; k += EXP_NT) ij[k - k0] = rowidx[k] | (colidx[k] << 16);
    __syncthreads();
    if (bl >= nb) return;          // (a lane beyond the batch: no barrier follows)
    const int b = b0 + bl;
    const bool copy = (adj[b] & 8) != 0;
    const double *const row = vf + (size_t)b * ldv;
    double *const o = out + b;
    const int run = (k1 - k0 + NSUB - 1) / NSUB, ks = k0 + sub * run, ke = min(k1, ks + run);
    if (copy) {          // (a loop of its own: a load beside the stores of the expansion would make every store wait for the one before)
        for (int k = ks; k < ke; k += EXP_U) {
            double t[EXP_U];
#pragma unroll
            for (int u = 0; u < EXP_U; u++) t[u] = row[min(k + u, ke - 1)];
#pragma unroll
            for (int u = 0; u < EXP_U; u++) if (k + u < ke) o[(size_t)(k + u) * B] = t[u];
        }
        return;
    }
    int jp = -1; double xj = 0.0, rj = 0.0;
    for (int k = ks; k < ke; k += EXP_U) {
        int e[EXP_U]; double vi[EXP_U], yi[EXP_U];
#pragma unroll
        for (int u = 0; u < EXP_U; u++) e[u] = ij[min(k + u, ke - 1) - k0];
#pragma unroll
        for (int u = 0; u < EXP_U; u++) { const int i = e[u] & 0xffff; vi[u] = vs[i * P + bl]; yi[u] = ys[i * P + bl]; }
#pragma unroll
        for (int u = 0; u < EXP_U; u++) {
            if (k + u >= ke) break;
            const int j = e[u] >> 16;
            if (j < n && j != jp) { jp = j; xj = xs[j * P + bl]; rj = -dq[j * sdqk + b * sdqb]; }
            o[(size_t)(k + u) * B] = (j < n) ? ce_dA_entry(xj, vi[u], yi[u], rj) : -vi[u];
        }
    }
}


// ================================================================================================
// parameter-map evaluation, batch-major:  out (B x rows) = P (B x cols) . map^T,  map in CSR (rows x cols)
// one thread per (row, instance); lanes walk rows -> coalesced 8-byte stores, gathers of P stay inside one instance's row
// ================================================================================================
// Parameter map with the instance's source row staged in LDS: one workgroup = one instance.  The source row (cols doubles) is
// read once, coalesced; every map row then gathers from LDS, so maps that transpose a matrix parameter (CSC order out of a
// row-major parameter, or back) cost one pass over HBM instead of a 16-fold over-fetch of partially used cache lines.
// ACC: out += (rows without entries are left untouched).
template <bool ACC>
__global__ void __launch_bounds__(512) k_parammap_lds(int rows, int cols, const int *__restrict__ indptr, const int *__restrict__ indices,
                                                      const double *__restrict__ vals, const double *__restrict__ P, long ldp,
                                                      double *__restrict__ out, long ldo) {
    extern __shared__ double pl[];
    constexpr int NT = 512, U = 4;
    const double *p = P + (size_t)blockIdx.x * ldp;
    double *o = out + (size_t)blockIdx.x * ldo;
    for (int c = threadIdx.x; c < cols; c += NT) pl[c] = p[c];
    __syncthreads();
    for (int r0 = threadIdx.x; r0 < rows; r0 += U * NT) {
        int t0[U], t1[U];
        bool single = true;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int r = r0 + u * NT;
            t0[u] = r < rows ? indptr[r] : 0;
            t1[u] = r < rows ? indptr[r + 1] : 0;
            single = single && (t1[u] - t0[u] <= 1);
        }
        if (single) {                                        // the common shape of a canonicalisation map: one entry per row
            double v[U]; int c[U];
#pragma unroll
            for (int u = 0; u < U; u++) { const bool on = t1[u] > t0[u]; v[u] = on ? vals[t0[u]] : 0.0; c[u] = on ? indices[t0[u]] : 0; }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int r = r0 + u * NT;
                const double a = t1[u] > t0[u] ? v[u] * pl[c[u]] : 0.0;      // (select: 0 * pl[0] would be NaN for a non-finite parameter 0)
                if (r < rows) { if (!ACC) o[r] = a; else if (t1[u] > t0[u]) o[r] += a; }
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int r = r0 + u * NT;
                if (r >= rows || (ACC && t0[u] == t1[u])) continue;
                double a = 0.0;
                for (int t = t0[u]; t < t1[u]; t++) a = fma(vals[t], pl[indices[t]], a);
                if (ACC) o[r] += a; else o[r] = a;
            }
        }
    }
}

template <int NB, bool ACC>
__global__ void __launch_bounds__(256) k_parammap(int rows, int B, const int *__restrict__ indptr, const int *__restrict__ indices,
                                                  const double *__restrict__ vals, const double *__restrict__ P, long ldp,
                                                  double *__restrict__ out, long ldo) {
    // one thread = one map row for NB consecutive instances: the row's (index, value) pairs are fetched once for NB gathers
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int b0 = blockIdx.y * NB;
    const int nb = min(NB, B - b0);
    const double *p = P + (size_t)b0 * ldp;
    const int t0 = indptr[r], t1 = indptr[r + 1];
    double a[NB];
#pragma unroll
    for (int u = 0; u < NB; u++) a[u] = 0.0;
    if (nb == NB) {
        for (int t = t0; t < t1; t++) {
            const double v = vals[t]; const int c = indices[t];
#pragma unroll
            for (int u = 0; u < NB; u++) a[u] = fma(v, p[(size_t)u * ldp + c], a[u]);
        }
#pragma unroll
        for (int u = 0; u < NB; u++) {
            double *o = out + (size_t)(b0 + u) * ldo + r;
            if (!ACC) *o = a[u]; else if (t1 > t0) *o += a[u];
        }
    } else {
        for (int u = 0; u < nb; u++) {
            double acc = 0.0;
            for (int t = t0; t < t1; t++) acc = fma(vals[t], p[(size_t)u * ldp + indices[t]], acc);
            double *o = out + (size_t)(b0 + u) * ldo + r;
            if (!ACC) *o = acc; else if (t1 > t0) *o += acc;
        }
    }
}

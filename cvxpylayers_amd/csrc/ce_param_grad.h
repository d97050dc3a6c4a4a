// ce_param_grad.h -- k_param_grad: the parameter gradient of K x B (cotangent, instance) pairs straight from the adjoint's factors: the transposed parameter
// maps applied to the entries of dA and to dq WITHOUT a dA row in memory (cone_engine.hip ce_vjp_many_params, ce_vjp_params; tests/test_gpu_param_grad.py)
#pragma once
#include "ce_dA_entry.h"       // ce_dA_entry, ce_db_entry, ce_dP_entry: the entries of the dA row and of dP, shared with k_backward_ns and k_expand_dA

// ================================================================================================
// g (K, B, rows) batch-major, written once:   g[p] = sum_e val_e . entry(i_e, j_e)  +  sum_e' val_e' . dq[j_e']
// ================================================================================================
// The map of a layer, composed once on the host (interfaces/param_grad.py): CSR over the rows = parameter columns 0 .. Ptot (the constant column included), the
// entries of the transposed A-map first, those of the transposed q-map behind them.  An entry is (code, k, val):
//   code >= 0: entry k of the value order, (i, j) = (code & 0xffff, code >> 16): ce_dA_entry(x_j, r_y,i, y_i, r_x,j) for j < n, ce_db_entry(y_i, r_tau, r_y,i) for j == n
//   code <  0, bit 30 clear: entry j = code & 0x3fffffff of the pair's dq row (k unused)
//   code <  0, bit 30 set: entry k of P's structure order (a native QP: ce_vjp_qp_many_params), (i, j) = (code & 0x7fff, code >> 15 & 0x7fff): ce_dP_entry(r_x,i, x_j, r_x,j,
//              x_i) = -1/2 (r_x,i x_j + r_x,j x_i), ONE share -- the doubling of a one-triangle structure and the frontend's symmetrisation are the host's, in val
// Every entry is rounded as the dA entry first and multiplied by val afterwards (one fma onto the running sum, which starts at zero): a row with one entry
// gets the bits of the product the parameter-map pass forms from a stored dA.
//
// Factors of pair (k, b), two conventions (mode):
//   PG_RECORDS  the record of k_backward_ns<MANY> / k_sa_lsqr's record mode at rec + k * srk + b * rpitch: r_y[0 .. m), r_tau, r_x[0 .. n)
//   PG_ROWHEAD  the single-cotangent adjoint's factor mode (K == 1): r_y at the head of row b of the batch-major dA workspace (rpitch = nnz_aug), r_tau = 0 and
//               r_x = -dq; adj[b] & 8: the LSQR re-solve wrote the WHOLE row there instead, and the entries are read from it (entry k of the value order)
//
// Shape of the work: a store stream of rows x 8 bytes per pair, fed by 2 n + 2 m + 1 factors and n + 1 dq entries per pair and a map that every pair shares.
//   grid.x: tiles of PG_TP consecutive pairs; grid.y: slabs of `slab` consecutive rows.  The workgroup stages the tile's x, y, r_y, r_x, dq and r_tau in LDS,
//   element-major ([element][pair], PG_TP = 16 doubles = 128 bytes per element: a lane fetches the eight pairs of a half tile with four 16-byte reads), so the map is
//   fetched once per PG_TP pairs, not once per instance.  Lanes run along the rows: a wave stores 64 consecutive doubles of one pair's g row, 512 contiguous bytes.
//   A row with more than PG_LONG entries (a scalar parameter that multiplies all of A has nnzA) is set aside in an LDS list and summed by the whole workgroup
//   behind the lane-per-row pass: lanes along the row's entries, a butterfly inside the wave, the four wave sums added in wave order -- a fixed order again.
//   Rows without an entry store 0.0.  No atomics on global memory: every g entry has one writer.
constexpr int PG_TP_MAX = 16, PG_NT = 256, PG_LONG = 32, PG_SU = 4;
// elements of one pair in LDS: x[n], y[m], r_y[m], r_x[n], dq[n + 1], r_tau
__host__ __device__ inline int pg_elems(int n, int m) { return 3 * n + 2 * m + 2; }
inline size_t param_grad_lds_bytes(int n, int m, int slab, int tp) {
    return sizeof(double) * ((size_t)pg_elems(n, m) * tp + (PG_NT / 64) * tp) + sizeof(int) * ((size_t)slab + tp + 2);
}

// PG_TP: pairs per tile, 16 where the tile fits LDS twice per CU, else 8, 4 or 2 (ce_tu_param_grad.hip); a lane works on half tiles of PG_HP <= 8 pairs
template <int PG_TP>
__global__ void __launch_bounds__(PG_NT) k_param_grad(CeParamGradArgs a) {
    constexpr int PG_HP = PG_TP < 8 ? PG_TP : 8;
    extern __shared__ __attribute__((aligned(16))) double pgs[];
    const int n = a.n, m = a.m, tid = threadIdx.x;
    double *xs = pgs, *ys = xs + (size_t)n * PG_TP, *vs = ys + (size_t)m * PG_TP, *rs = vs + (size_t)m * PG_TP, *ds = rs + (size_t)n * PG_TP;
    double *ts = ds + (size_t)(n + 1) * PG_TP, *red = ts + PG_TP;
    int *dense = (int *)(red + (PG_NT / 64) * PG_TP), *longs = dense + PG_TP + 2;
    __shared__ int nlong;          // (static: the atomic append below addresses LDS directly)
    const long npairs = (long)a.K * a.B, q0 = (long)blockIdx.x * PG_TP;
    const int np = (int)(npairs - q0 < PG_TP ? npairs - q0 : PG_TP);
    const int r0 = blockIdx.y * a.slab, r1 = min(a.rows, r0 + a.slab);
    // ---- stage the tile: PG_SU loads in flight per thread in front of the LDS writes; the pairs beyond the batch hold zeros (computed, never stored)
    auto stage = [&](double *dst, int cnt, auto &&src) __attribute__((always_inline)) {          // dst[e * PG_TP + p] = src(pair q0 + p, e) for e < cnt
        for (int i0 = tid; i0 < PG_TP * cnt; i0 += PG_SU * PG_NT) {
            double t[PG_SU];
#pragma unroll
            for (int u = 0; u < PG_SU; u++) {
                const int idx = i0 + u * PG_NT, p = idx / cnt, e = idx - p * cnt;
                t[u] = (idx < PG_TP * cnt && p < np) ? src(q0 + p, e) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < PG_SU; u++) { const int idx = i0 + u * PG_NT, p = idx / cnt, e = idx - p * cnt; if (idx < PG_TP * cnt) dst[e * PG_TP + p] = t[u]; }
        }
    };
    const bool rowhead = a.mode == PG_ROWHEAD;
    stage(xs, n, [&](long q, int e) { return a.x[(size_t)(q % a.B) * n + e]; });
    stage(ys, m, [&](long q, int e) { return a.y[(size_t)(q % a.B) * m + e]; });
    stage(ds, n + 1, [&](long q, int e) { const long k = q / a.B, b = q - k * a.B; return a.dq[k * a.sqK + e * a.sqk + b * a.sqb]; });
    if (rowhead) {
        stage(vs, m, [&](long q, int e) { return a.rec[(size_t)q * a.rpitch + e]; });
        stage(rs, n, [&](long q, int e) { return -a.dq[e * a.sqk + q * a.sqb]; });          // (K == 1: q is the instance)
    } else {
        stage(vs, m, [&](long q, int e) { const long k = q / a.B, b = q - k * a.B; return a.rec[k * a.srk + b * a.rpitch + e]; });
        stage(rs, n, [&](long q, int e) { const long k = q / a.B, b = q - k * a.B; return a.rec[k * a.srk + b * a.rpitch + m + 1 + e]; });
    }
    if (tid < PG_TP) {
        double rt = 0.0; int dn = 0;
        if (tid < np) {
            const long q = q0 + tid, k = q / a.B, b = q - k * a.B;
            if (rowhead) dn = (a.adj[q] & 8) != 0; else rt = a.rec[k * a.srk + b * a.rpitch + m];
        }
        ts[tid] = rt; dense[tid] = dn;
    }
    if (tid == 0) nlong = 0;
    __syncthreads();
    int anydense = 0;          // (bit p: pair p of the tile reads the row the re-solve wrote; uniform)
    if (rowhead) { for (int p = 0; p < PG_TP; p++) anydense |= dense[p] << p; }
    typedef const __attribute__((address_space(1))) double *gptr;          // (a.rec lives in a struct: named global here, so that no load is emitted as a flat one beside the LDS reads)
    const gptr rowg = (gptr)a.rec;
    // one entry of the map for the eight pairs of half tile h: e[u] = the dA entry / the dq entry of pair h * PG_HP + u
    auto entries = [&](int c, int kk, int h, double (&e)[PG_HP]) __attribute__((always_inline)) {
        const int o = h * PG_HP;
        if (c < 0) {
            if (c & 0x40000000) {          // (an entry of dP: x and r_x of the staged tile; never met in PG_ROWHEAD, whose kinds have no P)
                const int i = c & 0x7fff, j = (c >> 15) & 0x7fff;
                const double *xi = xs + (size_t)i * PG_TP + o, *xj = xs + (size_t)j * PG_TP + o, *ri = rs + (size_t)i * PG_TP + o, *rj = rs + (size_t)j * PG_TP + o;
#pragma unroll
                for (int u = 0; u < PG_HP; u++) e[u] = ce_dP_entry(ri[u], xj[u], rj[u], xi[u]);
                return;
            }
            const double *d = ds + (size_t)(c & 0x3fffffff) * PG_TP + o;
#pragma unroll
            for (int u = 0; u < PG_HP; u++) e[u] = d[u];
            return;
        }
        const int i = c & 0xffff, j = c >> 16;
        const double *yv = ys + (size_t)i * PG_TP + o, *vv = vs + (size_t)i * PG_TP + o;
        if (j < n) {
            const double *xv = xs + (size_t)j * PG_TP + o, *rv = rs + (size_t)j * PG_TP + o;
#pragma unroll
            for (int u = 0; u < PG_HP; u++) e[u] = ce_dA_entry(xv[u], vv[u], yv[u], rv[u]);
        } else {
#pragma unroll
            for (int u = 0; u < PG_HP; u++) e[u] = ce_db_entry(yv[u], ts[o + u], vv[u]);
        }
        if (anydense) {          // (PG_ROWHEAD, rare: the row the re-solve wrote stands for the factors of its instance)
            for (int u = 0; u < PG_HP; u++) if ((anydense >> (o + u)) & 1) e[u] = rowg[(size_t)(q0 + o + u) * a.rpitch + kk];
        }
    };
    // ---- lanes along the rows of the slab
    for (int r = r0 + tid; r < r1; r += PG_NT) {
        const int t0 = a.ptr[r], t1 = a.ptr[r + 1];
        if (t1 - t0 > PG_LONG) { longs[__hip_atomic_fetch_add(&nlong, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)] = r; continue; }
#pragma unroll
        for (int h = 0; h < PG_TP / PG_HP; h++) {
            double acc[PG_HP];
#pragma unroll
            for (int u = 0; u < PG_HP; u++) acc[u] = 0.0;
            for (int t = t0; t < t1; t++) {
                const double v = a.val[t];
                double e[PG_HP];
                entries(a.code[t], a.kidx[t], h, e);
#pragma unroll
                for (int u = 0; u < PG_HP; u++) acc[u] = fma(v, e[u], acc[u]);
            }
#pragma unroll
            for (int u = 0; u < PG_HP; u++) if (h * PG_HP + u < np) a.g[(size_t)(q0 + h * PG_HP + u) * a.rows + r] = acc[u];
        }
    }
    __syncthreads();
    // ---- the long rows of the slab, one after the other, lanes along the entries
    const int nl = nlong;
    for (int li = 0; li < nl; li++) {
        const int r = longs[li], t0 = a.ptr[r], t1 = a.ptr[r + 1];
#pragma unroll
        for (int h = 0; h < PG_TP / PG_HP; h++) {
            double acc[PG_HP];
#pragma unroll
            for (int u = 0; u < PG_HP; u++) acc[u] = 0.0;
            for (int t = t0 + tid; t < t1; t += PG_NT) {
                const double v = a.val[t];
                double e[PG_HP];
                entries(a.code[t], a.kidx[t], h, e);
#pragma unroll
                for (int u = 0; u < PG_HP; u++) acc[u] = fma(v, e[u], acc[u]);
            }
#pragma unroll
            for (int u = 0; u < PG_HP; u++) {
                for (int o = 32; o > 0; o >>= 1) acc[u] += __shfl_xor(acc[u], o);
                if ((tid & 63) == 0) red[(tid >> 6) * PG_TP + h * PG_HP + u] = acc[u];
            }
        }
        __syncthreads();
        if (tid < np) {
            double s = red[tid];
            for (int w = 1; w < PG_NT / 64; w++) s += red[w * PG_TP + tid];
            a.g[(size_t)(q0 + tid) * a.rows + r] = s;
        }
        __syncthreads();
    }
}

// ce_layout_kernels.h -- the layout pass (k_transpose) and the parameter-map products (k_parammap*) the host launches itself (cone_engine.hip; tests/test_gpu_layout_kernels.py)
#pragma once

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

// ce_value.h -- the optimal value of an instance and its envelope-theorem derivatives (cone_engine.hip ce_value, ce_value_jvp, ce_value_vjp; tests/test_gpu_value.py)
//
//   p*(theta) = c^T x + d + 1/2 x^T P x        at a solution (x, y) of   min c^T x + d + 1/2 x^T P x   s.t.  A x + s = b, s in K
// By the envelope theorem the derivative of p* is the PARTIAL derivative of the Lagrangian at (x, y): dp/dA = y x^T, dp/db = -y, dp/dc = x, dp/dd = 1,
// dp/dP = 1/2 x x^T.  No system is solved: the kernels below are products and sums over the template's structure.  In the boundary convention
// A_eval = [-A.data, b] (include/cone_engine.h):  dp/dA_eval[k] = -y_row x_col for an A entry, -y_row for a b entry.
// Not a tiled family: no row in ce_variants.h.  Plain C++, vector stores.
#pragma once

constexpr int VAL_NT = 256;        // threads of every kernel here
constexpr int VAL_IPB = 4;         // k_value_vjp_rows: instances per workgroup (the structure's row / column of an entry is fetched once for all of them)
constexpr int VAL_TI = 64;         // k_value_vjp_tile: instances per tile = lanes of a wave
constexpr int VAL_TLD = VAL_TI + 1;      // its LDS row pitch: the transposing writes of the staging loop land on 2 banks per 16 lanes instead of one

// Is the P structure one triangle?  Then an off-diagonal entry stands for both matrix entries (weight 2), the convention of ce_vjp_qp's dP.  Decided by every
// workgroup from the structure itself (the entry points take the structure as device arrays: no host copy to ask).  All threads of the workgroup call this.
__device__ inline bool val_one_triangle(const int *__restrict__ prow, const int *__restrict__ pcol, int nnz_p) {
    int up = 1, lo = 1;
    for (int k = threadIdx.x; k < nnz_p; k += VAL_NT) { const int r = prow[k], c = pcol[k]; up &= r <= c; lo &= r >= c; }
    up = __syncthreads_and(up); lo = __syncthreads_and(lo);
    return up || lo;
}

// sum of red[0 .. VAL_NT) in a fixed tree order; all threads call it, thread 0 holds the result
__device__ inline double val_tree_sum(double *red, double v) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = VAL_NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// One workgroup = one instance; every sum runs over the template's structure in an order fixed by the thread count alone (thread t takes entries t, t + 256, ...,
// then the tree above), so an instance's scalars depend neither on B nor on its position in the batch.
//   JVP = false:  pobj = c^T x + d + 1/2 x^T P x,   dobj = -b^T y - 1/2 x^T P x + d
//   JVP = true :  tval = tc^T x + td + 1/2 x^T tP x - sum_k tA_eval[k] (y_row x_col | y_row)
template <bool JVP>
__global__ void __launch_bounds__(VAL_NT) k_value(CeValueArgs a) {
    extern __shared__ double val_lds[];
    double *xs = val_lds, *ys = xs + a.n, *red = ys + a.m;
    const int i = blockIdx.x, t = threadIdx.x, n = a.n, m = a.m;
    for (int j = t; j < n; j += VAL_NT) xs[j] = a.x[(size_t)i * n + j];
    for (int r = t; r < m; r += VAL_NT) ys[r] = a.y[(size_t)i * m + r];
    const bool tri = a.nnz_p > 0 && val_one_triangle(a.prow, a.pcol, a.nnz_p);      // (its barriers also publish xs, ys)
    __syncthreads();
    const double *Pv = JVP ? a.tP : a.P;
    double quad = 0.0;
    if (Pv)
        for (int k = t; k < a.nnz_p; k += VAL_NT) {
            const int r = a.prow[k], c = a.pcol[k];
            if ((unsigned)r >= (unsigned)n || (unsigned)c >= (unsigned)n) continue;
            const double w = (tri && r != c) ? 1.0 : 0.5;
            quad = fma(w * Pv[(size_t)i * a.nnz_p + k], xs[r] * xs[c], quad);
        }
    if (JVP) {
        double acc = 0.0;
        if (a.tA)
            for (int k = t; k < a.nnz_aug; k += VAL_NT) {
                const int r = a.rowidx[k], c = a.colidx[k];
                const double yx = c < n ? ys[r] * xs[c] : ys[r];
                acc = fma(-a.tA[(size_t)i * a.stAb + k], yx, acc);
            }
        if (a.tq)
            for (int j = t; j <= n; j += VAL_NT) acc = fma(a.tq[j * a.stqk + i * a.stqb], j < n ? xs[j] : 1.0, acc);
        const double s = val_tree_sum(red, acc + quad);
        if (t == 0) a.tval[i] = s;
    } else {
        double lin = 0.0, bty = 0.0;
        for (int j = t; j < n; j += VAL_NT) lin = fma(a.q[j * a.sqk + i * a.sqb], xs[j], lin);
        for (int r = t; r < m; r += VAL_NT) { const int k = a.bpos[r]; if (k >= 0) bty = fma(a.A[k * a.sAk + i * a.sAb], ys[r], bty); }
        const double slin = val_tree_sum(red, lin), sq = val_tree_sum(red, quad), sb = val_tree_sum(red, bty);
        if (t == 0) {
            const double d = a.q[n * a.sqk + i * a.sqb];
            a.pobj[i] = (slin + d) + sq;
            a.dobj[i] = (-sb - sq) + d;
        }
    }
}

// The gradients for an upstream cotangent g (B), BATCH-MAJOR rows (sdAk == 1): the hot layout, the frontend's A_bm is native.  A workgroup stages x and -g y of
// VAL_IPB instances in LDS, its lanes run over the entries k and every wave stores whole 512-byte runs of a row.  Also writes dq (any stride pair) and the
// batch-major dP.  An instance with skip[i] != 0 gets exact zeros whatever its x, y, g hold (selects in front of the arithmetic: NaN never enters a product).
__global__ void __launch_bounds__(VAL_NT) k_value_vjp_rows(CeValueVjpArgs a) {
    extern __shared__ double val_lds[];
    const int n = a.n, m = a.m, t = threadIdx.x, i0 = blockIdx.x * VAL_IPB;
    double *xs = val_lds, *ys = xs + VAL_IPB * n, *gs = ys + VAL_IPB * m;       // ys = -g y
    if (t < VAL_IPB) {
        const int i = i0 + t;
        gs[t] = (i < a.B && !(a.skip && a.skip[i])) ? a.g[i] : 0.0;
    }
    __syncthreads();
    for (int u = 0; u < VAL_IPB; u++) {
        const int i = i0 + u;
        const bool on = i < a.B && !(a.skip && a.skip[i]);
        for (int j = t; j < n; j += VAL_NT) xs[u * n + j] = on ? a.x[(size_t)i * n + j] : 0.0;
        for (int r = t; r < m; r += VAL_NT) ys[u * m + r] = on ? -(gs[u] * a.y[(size_t)i * m + r]) : 0.0;
    }
    const bool tri = a.dP && a.nnz_p > 0 && val_one_triangle(a.prow, a.pcol, a.nnz_p);
    __syncthreads();
    const int nu = min(VAL_IPB, a.B - i0);
    if (a.dA && a.sdAk == 1)
        for (int k = t; k < a.nnz_aug; k += VAL_NT) {
            const int r = a.rowidx[k], c = a.colidx[k];
            for (int u = 0; u < nu; u++) a.dA[(size_t)(i0 + u) * a.sdAb + k] = c < n ? ys[u * m + r] * xs[u * n + c] : ys[u * m + r];
        }
    if (a.dq)
        for (int j = t; j <= n; j += VAL_NT)
            for (int u = 0; u < nu; u++) a.dq[j * a.sdqk + (i0 + u) * a.sdqb] = j < n ? gs[u] * xs[u * n + j] : gs[u];
    if (a.dP)
        for (int k = t; k < a.nnz_p; k += VAL_NT) {
            const int r = a.prow[k], c = a.pcol[k];
            const bool in = (unsigned)r < (unsigned)n && (unsigned)c < (unsigned)n;
            const double w = (tri && r != c) ? 1.0 : 0.5;
            for (int u = 0; u < nu; u++) a.dP[(size_t)(i0 + u) * a.nnz_p + k] = in ? (w * gs[u]) * (xs[u * n + r] * xs[u * n + c]) : 0.0;
        }
}

// dA in the BATCH-MINOR layout (sdAb == 1, the reference's (nnz_aug, B)): a tile of 64 instances, lanes over the instances, so a wave stores 512 contiguous bytes
// of one entry's row and no ce_transpose is needed behind the call.  Workgroup (tile, chunk) serves the entries [chunk * kchunk, (chunk + 1) * kchunk) of its tile;
// chunk 0 also writes dq when told to (wdq: sdqb == 1, the same coalescing).  STAGED: the tile's x and -g y sit in LDS, instance-minor with pitch VAL_TLD (the
// lanes of a wave read consecutive doubles); otherwise -- templates whose tile exceeds LDS -- the lanes gather them from global memory (L2).
template <bool STAGED>
__global__ void __launch_bounds__(VAL_NT) k_value_vjp_tile(CeValueVjpArgs a, int kchunk, int wdq) {
    extern __shared__ double val_lds[];
    const int n = a.n, m = a.m, t = threadIdx.x, i0 = blockIdx.x * VAL_TI;
    const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6), nw = VAL_NT / 64;
    const int i = i0 + lane;
    const bool on = i < a.B && !(a.skip && a.skip[i]);
    const double g = on ? a.g[i] : 0.0;
    double *xs = val_lds, *ys = xs + (size_t)n * VAL_TLD;
    if (STAGED) {
        // the tile's rows of x (and of y) are one contiguous range: coalesced reads, transposing LDS writes
        double *gt = ys + (size_t)m * VAL_TLD;
        if (t < VAL_TI) gt[lane] = g;
        __syncthreads();
        const int ni = min(VAL_TI, a.B - i0);
        for (int f = t; f < VAL_TI * n; f += VAL_NT) { const int u = f / n, j = f - u * n; xs[j * VAL_TLD + u] = (u < ni && !(a.skip && a.skip[i0 + u])) ? a.x[(size_t)i0 * n + f] : 0.0; }
        for (int f = t; f < VAL_TI * m; f += VAL_NT) { const int u = f / m, r = f - u * m; ys[r * VAL_TLD + u] = (u < ni && !(a.skip && a.skip[i0 + u])) ? -(gt[u] * a.y[(size_t)i0 * m + f]) : 0.0; }
        __syncthreads();
    }
    const int k0 = blockIdx.y * kchunk, k1 = min(a.nnz_aug, k0 + kchunk);
    if (a.dA)
        for (int k = k0 + wave; k < k1; k += nw) {
            const int r = a.rowidx[k], c = a.colidx[k];
            double v;
            if (STAGED) v = c < n ? ys[r * VAL_TLD + lane] * xs[c * VAL_TLD + lane] : ys[r * VAL_TLD + lane];
            else { const double gy = on ? -(g * a.y[(size_t)i * m + r]) : 0.0; v = c < n ? gy * (on ? a.x[(size_t)i * n + c] : 0.0) : gy; }
            if (i < a.B) a.dA[k * a.sdAk + i * a.sdAb] = v;
        }
    if (wdq && blockIdx.y == 0 && i < a.B)
        for (int j = wave; j <= n; j += nw) {
            double v = g;
            if (j < n) v = g * (STAGED ? xs[j * VAL_TLD + lane] : (on ? a.x[(size_t)i * n + j] : 0.0));
            a.dq[j * a.sdqk + i * a.sdqb] = v;
        }
}

// ce_check.h -- the forward kernels' termination test at a given point (cone_engine.hip ce_check_solved; tests/test_gpu_check_solved.py)
//
//   res_pri  = |A x + s - b|_inf        prl = max(|A x|_inf, |s|_inf, |b|_inf)
//   res_dual = |P x + A^T y + c|_inf    drl = max(|A^T y|_inf, |c|_inf, |P x|_inf)
//   gap      = |x^T P x + c^T x + b^T y|      grl = max(|c^T x|, |b^T y|, |x^T P x|)
//   solved  <=>  eligible, every number finite, and each of the three  <=  eps_abs + eps_rel * its scale        (ce_forward_v2.h's test at tau = 1)
// in the boundary convention A = -A_vals[A entries], b = A_vals[b entries] (0 on a row without one), c = q_vals[:n].  The cone conditions are NOT tested: the
// caller vouches for them (ce_refine returns complementary pairs in the cones by construction).
// One workgroup = one instance.  The instance's value row is read from memory once and staged in LDS when it fits (STAGED), so that the product by rows
// (A x: lanes over the rows) and the one by columns (A^T y: lanes over a column's entries) both read it conflict-free; a larger row is read twice, the second
// time from L2.  Every sum runs in an order fixed by the template and the thread count (chk_seg below, then wave butterflies and a fixed pass over the four
// waves): no floating-point atomics, an instance's numbers depend neither on B nor on its position in the batch.
// Not a tiled family: no row in ce_variants.h.  Plain C++, vector stores.
#pragma once

constexpr int CHK_NT = 256;        // threads of k_check_solved and k_check_count
constexpr int CHK_NW = CHK_NT / 64;
constexpr int CHK_NQ = 11;         // reduced quantities: 8 maxima, 3 sums

// Is the P structure one triangle?  (ce_value.h's rule and convention: an off-diagonal entry then stands for both matrix entries.)  All threads call this.
__device__ inline bool chk_one_triangle(const int *__restrict__ prow, const int *__restrict__ pcol, int nnz_p) {
    int up = 1, lo = 1;
    for (int k = threadIdx.x; k < nnz_p; k += CHK_NT) { const int r = prow[k], c = pcol[k]; up &= r <= c; lo &= r >= c; }
    up = __syncthreads_and(up); lo = __syncthreads_and(lo);
    return up || lo;
}

// One term a * b of a sum
struct ChkTerm { double a, b; };

// out[r] = sum over p in [ptr[r], ptr[r + 1])  (ptr null: [0, full))  of the terms f(r, p), for r < M.  G threads (a power of two <= CHK_NT) share a row: thread g
// takes p = lo + g, lo + g + G, ... in that order, the G partial sums are added in the order g = 0 .. G - 1.  GMINOR: the threads of a row are neighbours (their
// entries are: a column of the value row); otherwise the rows of neighbouring threads are (dense rows: neighbouring entries again).  The terms are fetched eight
// at a time -- index loads, then operands, all independent -- and added one after the other: the order of the sum is that of p.  All threads call this.
// (Measured at the metric shape: a wave per row with a butterfly over its lanes -- contiguous index loads, but one dependent chain of shuffles per row -- took
// 0.22 ms where this takes 0.13 ms.)
template <bool GMINOR, class F>
__device__ inline void chk_seg(int M, int G, const int *__restrict__ ptr, int full, double *red, double *out, F f) {
    constexpr int U = 8;
    const int t = threadIdx.x, R = CHK_NT / G;
    const int lr = GMINOR ? t / G : t % R, g = GMINOR ? t % G : t / R, gs = GMINOR ? 1 : R;
    for (int base = 0; base < M; base += R) {
        const int r = base + lr;
        double acc = 0.0;
        if (r < M) {
            const int lo = ptr ? ptr[r] : 0, hi = ptr ? ptr[r + 1] : full;
            int p = lo + g;
            for (; p + (U - 1) * G < hi; p += U * G) {
                ChkTerm w[U];
#pragma unroll
                for (int u = 0; u < U; u++) w[u] = f(r, p + u * G);
#pragma unroll
                for (int u = 0; u < U; u++) acc = fma(w[u].a, w[u].b, acc);
            }
            for (; p < hi; p += G) { const ChkTerm w = f(r, p); acc = fma(w.a, w.b, acc); }
        }
        red[t] = acc;
        __syncthreads();
        if (g == 0 && r < M) {
            double sum = red[t];
            for (int u = 1; u < G; u++) sum += red[t + u * gs];
            out[r] = sum;
        }
        __syncthreads();
    }
}

template <bool STAGED>
__global__ void __launch_bounds__(CHK_NT) k_check_solved(CeCheckArgs a) {
    extern __shared__ double chk_lds[];
    const int i = blockIdx.x, t = threadIdx.x, n = a.n, m = a.m;
    if (a.eligible && !(a.eligible[i] & a.emask)) {          // (the same answer in every thread: the whole workgroup leaves)
        if (t == 0) a.solved[i] = 0;
        return;
    }
    double *xs = chk_lds, *ys = xs + n, *ss = ys + m, *ax = ss + m, *aty = ax + m, *px = aty + n, *red = px + n, *wred = red + CHK_NT, *av = wred + CHK_NW * CHK_NQ;
    int bad = 0;
    for (int j = t; j < n; j += CHK_NT) { const double v = a.x[(size_t)i * n + j]; xs[j] = v; bad |= !isfinite(v); }
    for (int r = t; r < m; r += CHK_NT) {
        const double v = a.y[(size_t)i * m + r], w = a.s[(size_t)i * m + r];
        ys[r] = v; ss[r] = w; bad |= !isfinite(v) || !isfinite(w);
    }
    const double *Ai = a.A + (long)i * a.sAb;
    if (STAGED) {          // eight loads in flight per thread before the first LDS store waits for one
        int k = t;
        for (; k + 7 * CHK_NT < a.nnz_aug; k += 8 * CHK_NT) {
            double w[8];
#pragma unroll
            for (int u = 0; u < 8; u++) w[u] = Ai[(long)(k + u * CHK_NT) * a.sAk];
#pragma unroll
            for (int u = 0; u < 8; u++) av[k + u * CHK_NT] = w[u];
        }
        for (; k < a.nnz_aug; k += CHK_NT) av[k] = Ai[(long)k * a.sAk];
    }
    const bool tri = a.nnz_p > 0 && chk_one_triangle(a.prow, a.pcol, a.nnz_p);
    __syncthreads();
    auto val = [&](int k) -> double { return STAGED ? av[k] : Ai[(long)k * a.sAk]; };
    // A x by rows (CSR of the A part: column and value position of every entry), A^T y by columns (the value order itself is CSC), P x by a scan of the structure
    chk_seg<false>(m, a.gr, a.rptr, 0, red, ax, [&](int, int p) { return ChkTerm{-val(a.rsrc[p]), xs[a.rcol[p]]}; });
    chk_seg<true>(n, a.gc, a.cptr, 0, red, aty, [&](int, int k) { return ChkTerm{-val(k), ys[a.rowidx[k]]}; });
    if (a.nnz_p > 0) {
        const double *Pi = a.P + (size_t)i * a.nnz_p;
        // (an entry that does not touch row j, or lies out of range, adds P_k * 0)
        chk_seg<true>(n, a.gc, nullptr, a.nnz_p, red, px, [&](int j, int k) {
            const int r = a.prow[k], c = a.pcol[k];
            const bool in = (unsigned)r < (unsigned)n && (unsigned)c < (unsigned)n;
            const int other = r == j ? c : ((tri && c == j) ? r : -1);
            return ChkTerm{Pi[k], (in && other >= 0) ? xs[other] : 0.0};
        });
    }
    // 0 res_pri, 1 |A x|, 2 |s|, 3 |b|, 4 res_dual, 5 |A^T y|, 6 |c|, 7 |P x| (maxima);  8 c^T x, 9 b^T y, 10 x^T P x (sums)
    double v[CHK_NQ];
    for (int u = 0; u < CHK_NQ; u++) v[u] = 0.0;
    for (int r = t; r < m; r += CHK_NT) {
        const int kb = a.bpos[r];
        const double b = kb >= 0 ? val(kb) : 0.0, axr = ax[r], sr = ss[r];
        bad |= !isfinite(b) || !isfinite(axr);
        v[0] = fmax(v[0], fabs((axr + sr) - b)); v[1] = fmax(v[1], fabs(axr)); v[2] = fmax(v[2], fabs(sr)); v[3] = fmax(v[3], fabs(b));
        v[9] = fma(b, ys[r], v[9]);
    }
    for (int j = t; j < n; j += CHK_NT) {
        const double c = a.q[(long)j * a.sqk + (long)i * a.sqb], atyj = aty[j], pxj = a.nnz_p > 0 ? px[j] : 0.0;
        bad |= !isfinite(c) || !isfinite(atyj) || !isfinite(pxj);
        v[4] = fmax(v[4], fabs((pxj + atyj) + c)); v[5] = fmax(v[5], fabs(atyj)); v[6] = fmax(v[6], fabs(c)); v[7] = fmax(v[7], fabs(pxj));
        v[8] = fma(c, xs[j], v[8]); v[10] = fma(pxj, xs[j], v[10]);
    }
    for (int off = 1; off < 64; off <<= 1)
        for (int u = 0; u < CHK_NQ; u++) { const double o = __shfl_xor(v[u], off); v[u] = u < 8 ? fmax(v[u], o) : v[u] + o; }
    if ((t & 63) == 0)
        for (int u = 0; u < CHK_NQ; u++) wred[(t >> 6) * CHK_NQ + u] = v[u];
    bad = __syncthreads_or(bad);          // (also publishes wred)
    if (t != 0) return;
    for (int w = 1; w < CHK_NW; w++)
        for (int u = 0; u < CHK_NQ; u++) { const double o = wred[w * CHK_NQ + u]; v[u] = u < 8 ? fmax(v[u], o) : v[u] + o; }
    const double res_pri = v[0], res_dual = v[4], gap = fabs((v[10] + v[8]) + v[9]);
    const double prl = fmax(fmax(v[3], v[2]), v[1]), drl = fmax(fmax(v[6], v[5]), v[7]), grl = fmax(fmax(fabs(v[8]), fabs(v[9])), fabs(v[10]));
    const bool ok = !bad && isfinite(res_pri) && isfinite(res_dual) && isfinite(gap) && isfinite(prl) && isfinite(drl) && isfinite(grl) &&
                    res_pri <= a.eps_abs + a.eps_rel * prl && res_dual <= a.eps_abs + a.eps_rel * drl && gap <= a.eps_abs + a.eps_rel * grl;
    a.solved[i] = ok ? 1 : 0;
    if (ok) {
        a.status[i] = 1; a.iters[i] = 0;
        a.resid[(size_t)3 * i] = res_pri; a.resid[(size_t)3 * i + 1] = res_dual; a.resid[(size_t)3 * i + 2] = gap;
    }
}

// n_unsolved[0] = number of zero bytes of solved[0 .. B): one workgroup, integer sums (set, not accumulated)
__global__ void __launch_bounds__(CHK_NT) k_check_count(int B, const unsigned char *__restrict__ solved, int *n_unsolved) {
    __shared__ int cnt[CHK_NT];
    const int t = threadIdx.x;
    int c = 0;
    for (int i = t; i < B; i += CHK_NT) c += solved[i] ? 0 : 1;
    cnt[t] = c;
    __syncthreads();
    for (int s = CHK_NT / 2; s > 0; s >>= 1) {
        if (t < s) cnt[t] += cnt[t + s];
        __syncthreads();
    }
    if (t == 0) n_unsolved[0] = cnt[0];
}

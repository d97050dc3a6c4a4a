"""Shared by test_gpu_psd_jvp.py, test_gpu_psd_ns_refine.py, test_gpu_psd_ns_layer.py and test_psd_ns_layout_host.py: the shapes, instances and dense numpy
references of the search-free elimination with PSD blocks (k_backward_ns<..., PSD> behind ce_jvp_psd / ce_refine_psd).  Nothing here needs a GPU until an engine
is asked for.

Instances: P.generate(n, cones, B, seed) at the oracle's point (eps 1e-10, max_iters 200 000).  Dense references as tri_ns_kit builds its own, per instance, in
solver form (A x + s = b), v = y - s, D = DPi(v) on the dual cone -- test_gpu_refine._proj for the zero / nonnegative / second-order rows; for a PSD block
smat(v_c) = U Lambda U^T by numpy.linalg.eigh and, in the basis E_ab = svec(sym(u_a u_b^T)), the eigenvalue B_ab of D: 1 when both eigenvalues are positive, 0
when both are non-positive, l+ / (l+ - l-) otherwise:
    [[0, A^T D], [A, D - I]] (d_x, d_v) = -(g_x, g_y),   g_x = tA^T y + tc,   g_y = tA x - tb,   dx = d_x, dy = D d_v, ds = (D - I) d_v
and the same matrix with the KKT residual (F_x = A^T y^ + c, F_y = A x + s^ - b) on the right for one Newton step.

Checked on the CPU with the oracle for these exact shapes and seeds: every instance is Solved; no instance has a weighted PSD row with 1 - B < 1e-5 (the smallest
min(B, 1 - B) over all shapes is 3.4e-4), so the stiff rule flags nothing; the dense systems have condition numbers <= 2.1e2 (psd_small), 3.0e2 (psd_mixed),
3.1e2 (psd_only), 2.0e2 (lqr_like), 3.0e4 (row2_n80), so the <= 1e11 filter leaves nothing out; psd_mixed holds blocks in all three states (all eigenvalues
positive 1, all non-positive 3, mixed 92) and so does psd_only (2 / 6 / 88); at most 16 weighted rows per instance.  Together: orders 2 to 8, an odd order (a bye
in the Jacobi tournament), an order with k^2 > 64 (the rotation's lane stride), two blocks of different order (the maxs pitch), a block as the last rows."""
import numpy as np

from cvxpylayers_amd import problems as P

# name -> (n, cones, B, seed)
SHAPES = {
    "psd_small": (4, {"z": 1, "s": [3]}, 16, 1),
    "psd_mixed": (12, {"z": 2, "l": 4, "q": [4], "s": [3, 4]}, 48, 1),
    "psd_only": (10, {"s": [4, 2, 3]}, 32, 5),
    "lqr_like": (24, {"z": 3, "l": 2, "s": [6, 4]}, 32, 3),
    "row2_n80": (80, {"z": 4, "l": 10, "q": [11, 11], "s": [8, 5]}, 24, 7),
}
_POINTS: dict = {}


def plain_part(cones):
    return {"z": cones.get("z", 0), "l": cones.get("l", 0), "q": list(cones.get("q", []))}


def plain_rows(cones):
    return cones.get("z", 0) + cones.get("l", 0) + sum(cones.get("q", []))


def m_of(cones):
    return plain_rows(cones) + sum(k * (k + 1) // 2 for k in cones.get("s", []))


def blocks(cones):
    """[(first row, order)] of the PSD blocks in row order (z, l, q, s; no triple in these templates)"""
    out, o = [], plain_rows(cones)
    for k in cones.get("s", []):
        out.append((o, k)); o += k * (k + 1) // 2
    return out


def smat(w, k):
    """the symmetric matrix of a svec: lower triangle, column-major, off-diagonals times sqrt 2 (oracle/cone_oracle.c)"""
    M = np.zeros((k, k)); pos = 0
    for b in range(k):
        for a in range(b, k):
            M[a, b] = M[b, a] = w[pos] if a == b else w[pos] / np.sqrt(2.0)
            pos += 1
    return M


def svec(M):
    k = M.shape[0]
    return np.array([M[a, b] if a == b else M[a, b] * np.sqrt(2.0) for b in range(k) for a in range(b, k)])


def block_eig(w, k):
    """(U, Lambda, Q, B) of one block: smat(w) = U Lambda U^T, the orthonormal basis Q (columns E_ab in svec order) and the eigenvalue B_ab of D Pi per column"""
    lam, U = np.linalg.eigh(smat(w, k))
    cols, Bv = [], []
    for b in range(k):
        for a in range(b, k):
            E = 0.5 * (np.outer(U[:, a], U[:, b]) + np.outer(U[:, b], U[:, a]))
            cols.append(svec(E if a == b else E * np.sqrt(2.0)))
            la, lb = lam[a], lam[b]
            Bv.append(1.0 if (la > 0 and lb > 0) else (0.0 if (la <= 0 and lb <= 0) else max(la, lb) / (max(la, lb) - min(la, lb))))
    return U, lam, np.array(cols).T, np.array(Bv)


def proj(v, cones):
    """projection of one v onto the dual cone and its derivative D: the plain rows by test_gpu_refine._proj, the PSD blocks by eigh and the B_ab rule"""
    from test_gpu_refine import _proj
    o = plain_rows(cones)
    m = v.size
    out = v.copy(); D = np.zeros((m, m))
    out[:o], D[:o, :o] = _proj(v[:o], plain_part(cones))
    for r0, k in blocks(cones):
        d = k * (k + 1) // 2
        U, lam, Q, Bv = block_eig(v[r0:r0 + d], k)
        out[r0:r0 + d] = svec((U * np.maximum(lam, 0.0)) @ U.T)
        D[r0:r0 + d, r0:r0 + d] = (Q * Bv) @ Q.T
    return out, D


def block_states(v, cones):
    """per block of one v: 0 all eigenvalues positive (D = I), 1 all non-positive (D = 0), 2 mixed; and the smallest min(B, 1 - B) over its weighted rows (1: none)"""
    kinds, margin = [], 1.0
    for r0, k in blocks(cones):
        _, lam, _, Bv = block_eig(v[r0:r0 + k * (k + 1) // 2], k)
        kinds.append(0 if (lam > 0).all() else (1 if (lam <= 0).all() else 2))
        mix = Bv[(Bv != 0.0) & (Bv != 1.0)]
        if mix.size:
            margin = min(margin, float(np.minimum(mix, 1 - mix).min()))
    return kinds, margin


def state_counts(name):
    """(blocks with D = I, with D = 0, mixed) over the shape's instances, the smallest margin min(B, 1 - B) of a weighted row, the largest weighted-row count"""
    _, cones, _, _, _, ref = problem(name)
    counts, margin, kw = [0, 0, 0], 1.0, 0
    for i in range(ref["x"].shape[0]):
        v = ref["y"][i] - ref["s"][i]
        kinds, mg = block_states(v, cones)
        for k in kinds:
            counts[k] += 1
        margin = min(margin, mg)
        nw = 0
        for r0, k in blocks(cones):
            Bv = block_eig(v[r0:r0 + k * (k + 1) // 2], k)[3]
            nw += int(((Bv != 0.0) & (Bv != 1.0)).sum())
        kw = max(kw, nw)
    return tuple(counts), margin, kw


def residual(A, b, c, x, v, cones):
    """(F_x, F_y, y-hat, D) of one instance at (x, v)"""
    yh, D = proj(v, cones)
    return A.T @ yh + c, A @ x + (yh - v) - b, yh, D


def kkt_matrix(A, D):
    m, n = A.shape
    return np.block([[np.zeros((n, n)), A.T @ D], [A, D - np.eye(m)]])


def dense_jvp(A, x, y, s, tA, tb, tc, cones):
    """(dx, dy, ds, well conditioned, condition numbers) of every instance by a dense solve of the system in the module docstring"""
    B, m, n = A.shape
    out = np.zeros((B, n)), np.zeros((B, m)), np.zeros((B, m)); ok = np.zeros(B, bool); cond = np.zeros(B)
    for i in range(B):
        _, D = proj(y[i] - s[i], cones)
        J = kkt_matrix(A[i], D)
        gx = tA[i].T @ y[i] + tc[i]; gy = tA[i] @ x[i] - tb[i]
        cond[i] = np.linalg.cond(J) if np.isfinite(J).all() else np.inf
        if not cond[i] <= 1e11:
            continue
        d = np.linalg.solve(J, -np.concatenate([gx, gy]))
        ok[i] = True
        out[0][i] = d[:n]; out[1][i] = D @ d[n:]; out[2][i] = (D - np.eye(m)) @ d[n:]
    return out + (ok, cond)


def dense_newton(A, b, c, x, v, cones, longdouble=False):
    """(dx, dv, well conditioned) of one Newton step on the KKT residual of every instance; longdouble: the residual and one step of iterative refinement of the
    solve in extended precision"""
    B, m, n = A.shape
    dx = np.zeros((B, n)); dv = np.zeros((B, m)); ok = np.zeros(B, bool)
    for i in range(B):
        fx, fy, yh, D = residual(A[i], b[i], c[i], x[i], v[i], cones)
        J = kkt_matrix(A[i], D)
        if not np.isfinite(J).all() or np.linalg.cond(J) > 1e11:
            continue
        if longdouble:
            L = np.longdouble
            Al, yl, vl, xl = (np.asarray(t, dtype=L) for t in (A[i], yh, v[i], x[i]))
            rhs = -np.concatenate([Al.T @ yl + c[i].astype(L), Al @ xl + (yl - vl) - b[i].astype(L)])
            d = np.linalg.solve(J, rhs.astype(np.float64)).astype(L)
            d = d + np.linalg.solve(J, (rhs - J.astype(L) @ d).astype(np.float64)).astype(L)
            d = d.astype(np.float64)
        else:
            d = np.linalg.solve(J, -np.concatenate([fx, fy]))
        ok[i] = True; dx[i], dv[i] = d[:n], d[n:]
    return dx, dv, ok


def rho(A, b, c, x, y, s):
    """rho of every instance at the arrays as given (include/cone_engine.h ce_refine), in extended precision"""
    from test_gpu_refine import _rho
    return _rho(A, b, c, x, y, s)


def problem(name):
    """(n, cones, A, b, c, the oracle's solution at eps 1e-10) of a shape: computed once, shared, not changed"""
    if name not in _POINTS:
        from oracle import oracle
        n, cones, B, seed = SHAPES[name]
        A, b, c = P.generate(n, cones, B, seed=seed)
        _POINTS[name] = (n, cones, A, b, c, oracle.solve_batch(A, b, c, cones, eps=1e-10, max_iters=200000))
    return _POINTS[name]


def plant_stiff_block(y, s, cones, inst, seed=0):
    """copies of (y, s) with instance `inst`'s first PSD block replaced by a stiff one: v_c = U diag(1, ..., 1, -3e-7) U^T for a random orthogonal U, so that the rows
    (a, last) have 1 - B = 3e-7 / (1 + 3e-7) < 1e-5.  The point need not be optimal: the derivative system is linear algebra at the point given."""
    r0, k = blocks(cones)[0]
    d = k * (k + 1) // 2
    rng = np.random.default_rng(seed)
    U, _ = np.linalg.qr(rng.standard_normal((k, k)))
    lam = np.ones(k); lam[-1] = -3e-7
    V = (U * lam) @ U.T
    Vp = (U * np.maximum(lam, 0.0)) @ U.T
    y, s = y.copy(), s.copy()
    y[inst, r0:r0 + d] = svec(Vp); s[inst, r0:r0 + d] = svec(Vp - V)
    return y, s


# ---------------------------------------------------------------------------------------------- the layout and the plan on the host (g++, no GPU)
HOST_SRC = r'''
#include <cstdio>
#include "ce_plan.h"
extern "C" {
// the kernel's carve (ce_backward_ns.h, PSD), restated with integer offsets: doubles from sm, then ints from (int *)sm, then the blocks' doubles.
// out: first byte of psdU, psdEv, lamp, psdScr, psdXW, end of the carve
void h_carve_psd(int n, int m, int nq, int ns, int maxs, int psdrows, int NTILE, int NTHR, long *out) {
    const int NWB = NTHR / 64, nqs = nq > 0 ? nq : 1, npad = n + (n & 1), KWMAX = bwd_ns_kwmax(m), lda = n;
    long p = 0;
    p += (long)m * lda; p += p & 1;
    p += m; p += m; p += npad; p += npad; p += npad; p += 5 * nqs; p += KWMAX; p += KWMAX; p += NWB * 8; p += nqs;
    p += p & 1;
    p += bwd_ns_union_doubles(n, m, nqs, NTILE);
    long ip = 2 * p;
    ip += m; ip += m; ip += nqs; ip += nqs; ip += nqs; ip += n; ip += n; ip += n; ip += n; ip += KWMAX; ip += KWMAX; ip += NWB + 1; ip += 8;
    ip += ip & 1;
    long q = ip / 2;
    out[0] = 8 * q; q += (long)ns * maxs * maxs;
    out[1] = 8 * q; q += (long)ns * maxs;
    out[2] = 8 * q; q += psdrows;
    out[3] = 8 * q; q += 2L * maxs * maxs + 2 * maxs + 8;
    out[4] = 8 * q; q += 2L * NWB * maxs * maxs;
    out[5] = 8 * q;
}
// out: (first byte, byte count) of every segment of the PSD mode in the struct's order -- doubles, the union and its five members, ints, the five PSD segments --
// then the first byte of slack and the footprint; n_seg pairs
int h_layout_psd(int n, int m, int nq, int ns, int maxs, int psdrows, int NTILE, int NTHR, long *out) {
    const NsLayout L = ns_layout(n, m, nq, NTILE, NTHR, false, 0, ns, maxs, psdrows);
    const NsSeg dbl[] = {L.A, L.vv, L.dv, L.rx, L.fvec, L.dB, L.cinfo, L.tvec, L.wgt, L.red, L.qaz, L.U, L.az, L.pub, L.Rbuf, L.qv2, L.mu};
    const NsSeg ints[] = {L.rkind, L.eqrow, L.ckind, L.ceq, L.cbase, L.erow, L.pcol, L.cmap, L.fcol, L.wrow, L.wsrc, L.wcnt, L.misc};
    const NsSeg psd[] = {L.psdU, L.psdEv, L.lamp, L.psdScr, L.psdXW};
    int k = 0;
    for (const NsSeg &s : dbl) { out[2 * k] = 8L * s.off; out[2 * k + 1] = 8L * s.len; k++; }
    for (const NsSeg &s : ints) { out[2 * k] = 4L * s.off; out[2 * k + 1] = 4L * s.len; k++; }
    for (const NsSeg &s : psd) { out[2 * k] = 8L * s.off; out[2 * k + 1] = 8L * s.len; k++; }
    out[2 * k] = 4L * L.slack.off; out[2 * k + 1] = (long)L.bytes;
    return k;
}
// out: the plain, QP and TRI (ntri triples) footprints, the PSD one, and the PSD / QP / TRI segment lengths of the three other modes added up (0)
void h_footprints(int n, int m, int nq, int ntri, int ns, int maxs, int psdrows, int NTILE, int NTHR, long *out) {
    out[0] = (long)bwd_ns_lds_bytes_of(n, m, nq, NTILE, NTHR); out[1] = (long)bwd_ns_qp_lds_bytes_of(n, m, nq, NTILE, NTHR);
    out[2] = (long)bwd_ns_tri_lds_bytes_of(n, m, nq, ntri, NTILE, NTHR); out[3] = (long)bwd_ns_psd_lds_bytes_of(n, m, nq, ns, maxs, psdrows, NTILE, NTHR);
    long z = 0;
    for (const NsLayout &L : {ns_layout(n, m, nq, NTILE, NTHR, false), ns_layout(n, m, nq, NTILE, NTHR, true), ns_layout(n, m, nq, NTILE, NTHR, false, ntri)})
        z += L.psdU.len + L.psdEv.len + L.lamp.len + L.psdScr.len + L.psdXW.len;
    out[4] = z;
}
void h_row(int v, int *ntile, int *nthr) { *ntile = NS_ROWS[v].NTILE; *nthr = NS_ROWS[v].NTHR; }
int h_rows() { return (int)std::size(NS_ROWS); }
// out: ns_variant, qp_ns_variant, tri_ns_variant, psd_ns_variant, psd_ns_lds, bwd_mode, brt_variant, ns_lds, qp_ns_lds, tri_ns_lds
int h_plan_psd(const ce_template *tpl, long *out) {
    DevT T{}; std::vector<int> qoff, soff; CePlan P;
    plan_sizes(tpl, T, qoff, soff);
    const int rc = plan_engine(tpl, T, tpl->nnz_p, read_plan_env(), P);
    if (rc) return rc;
    out[0] = P.ns_variant; out[1] = P.qp_ns_variant; out[2] = P.tri_ns_variant; out[3] = P.psd_ns_variant; out[4] = (long)P.psd_ns_lds; out[5] = P.bwd_mode;
    out[6] = P.brt_variant; out[7] = (long)P.ns_lds; out[8] = (long)P.qp_ns_lds; out[9] = (long)P.tri_ns_lds;
    return 0;
}
}
'''
HOST_PLAN_FIELDS = ("ns_variant", "qp_ns_variant", "tri_ns_variant", "psd_ns_variant", "psd_ns_lds", "bwd_mode", "brt_variant", "ns_lds", "qp_ns_lds", "tri_ns_lds")
PLAN_ENV = ("CE_FWD", "CE_FORCE_GENERIC", "CE_BWD_NS", "CE_GEN_BLOCKED", "CE_WL", "CE_F2_NEUMANN", "CE_BWD_TWO_TILE", "CE_BWD_FAST_VARIANT")
_HOST: dict = {}


def host_lib():
    """csrc/ce_plan.h and csrc/ce_ns_layout.h behind the shim above, compiled once per process with g++ into a temporary directory"""
    if "lib" not in _HOST:
        import ctypes as C
        import os
        import subprocess
        import tempfile
        from cvxpylayers_amd import _lib
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        _HOST["dir"] = tempfile.TemporaryDirectory(prefix="psd_ns_host_")
        src, so = os.path.join(_HOST["dir"].name, "host.cpp"), os.path.join(_HOST["dir"].name, "libpsd_ns_host.so")
        with open(src, "w") as f:
            f.write(HOST_SRC)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__host__=", "-D__device__=", "-shared", "-fPIC", "-I", os.path.join(root, "cvxpylayers_amd", "csrc"),
                               "-I", os.path.join(root, "include"), "-o", so, src])
        L = C.CDLL(so)
        L.h_carve_psd.argtypes = [C.c_int] * 8 + [C.POINTER(C.c_long)]; L.h_carve_psd.restype = None
        L.h_layout_psd.argtypes = [C.c_int] * 8 + [C.POINTER(C.c_long)]
        L.h_footprints.argtypes = [C.c_int] * 9 + [C.POINTER(C.c_long)]; L.h_footprints.restype = None
        L.h_row.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.h_plan_psd.argtypes = [C.POINTER(_lib.CeTemplate), C.POINTER(C.c_long)]
        _HOST["lib"] = L
    return _HOST["lib"]


def host_plan(n, cones, nnz_p=0):
    """{HOST_PLAN_FIELDS} of a template from the g++ build of the plan (the switches are read from the environment, as ce_create reads them); None when refused"""
    import ctypes as C
    from cvxpylayers_amd import _lib
    tpl = P.dense_template(n, cones)
    keep = [np.ascontiguousarray(tpl.indices, dtype=np.int32), np.ascontiguousarray(tpl.indptr, dtype=np.int32), np.ascontiguousarray(cones.get("q", []), dtype=np.int32),
            np.ascontiguousarray(cones.get("s", []), dtype=np.int32), np.ascontiguousarray(cones.get("p", []), dtype=np.float64)]
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))          # noqa: E731
    t = _lib.CeTemplate()
    t.n, t.m, t.nnz_aug, t.indices, t.indptr = int(tpl.n), int(tpl.m), int(keep[1][-1]), ip(keep[0]), ip(keep[1])
    t.z, t.l, t.nq, t.q, t.ns, t.s = int(cones.get("z", 0)), int(cones.get("l", 0)), len(keep[2]), ip(keep[2]), len(keep[3]), ip(keep[3])
    t.nep, t.np, t.p = int(cones.get("ep", 0)), len(keep[4]), keep[4].ctypes.data_as(C.POINTER(C.c_double))
    if nnz_p:
        keep += [np.ascontiguousarray([i for j in range(n) for i in range(j + 1)], dtype=np.int32), np.ascontiguousarray(np.cumsum([0] + list(range(1, n + 1))), dtype=np.int32)]
        t.nnz_p, t.p_indices, t.p_indptr = int(keep[6][-1]), ip(keep[5]), ip(keep[6])
    out = (C.c_long * len(HOST_PLAN_FIELDS))()
    return dict(zip(HOST_PLAN_FIELDS, out)) if host_lib().h_plan_psd(C.byref(t), out) == 0 else None

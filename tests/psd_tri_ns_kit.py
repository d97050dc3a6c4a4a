"""Shared by the test_gpu_psd_tri_*.py files and test_psd_tri_ns_layout_host.py: the shapes, instances and dense numpy references of the search-free elimination on
templates with PSD blocks AND exponential / power triples (k_backward_ns<..., TRI, ..., PSD> behind ce_jvp_psd_tri, ce_refine_psd_tri, ce_vjp_psd_tri_many,
ce_jvp_psd_tri_many).  Nothing here needs a GPU until an engine is asked for.

Instances: P.generate(n, cones, B, seed) at the oracle's point (eps 1e-10, max_iters 200 000).  Row order z, l, q, s, ep, p.  Dense references per instance in
solver form (A x + s = b), v = y - s, D = DPi(v) on the dual cone: the plain rows by test_gpu_refine._proj, the blocks by psd_ns_kit.block_eig (eigh and the B_ab
rule), the triples by the oracle's dproj_exp / dproj_pow with dual=True:
    [[0, A^T D], [A, D - I]] (d_x, d_v) = -(g_x, g_y),   g_x = tA^T y + tc,   g_y = tA x - tb,   dx = d_x, dy = D d_v, ds = (D - I) d_v
and the same matrix with the KKT residual (F_x = A^T y^ + c, F_y = A x + s^ - b) on the right for one Newton step.

Checked on the CPU with the oracle for these exact shapes and seeds: every instance is Solved; the smallest min(B, 1 - B) of a weighted PSD row is 2.9e-4
(row2_n80) and the smallest margin of a triple's middle eigenvalue 4.9e-3 (mix_all), so the stiff rule flags nothing from either kind; the dense systems have
condition numbers <= 5.9e3, so the <= 1e11 filter leaves nothing out; psd_tri_only holds blocks in all three states (2 / 8 / 54) and triples in all three
(10 / 16 / 70); at most 28 weighted rows per instance (row2_n80)."""
import numpy as np

import psd_ns_kit as PK
from cvxpylayers_amd import problems as P

# name -> (n, cones, B, seed)
SHAPES = {
    "mix_small": (6, {"z": 1, "l": 2, "s": [2], "ep": 1}, 16, 1),
    "mix_all": (14, {"z": 2, "l": 4, "q": [4], "s": [3, 4], "ep": 2, "p": [0.3, -0.6]}, 48, 1),
    "psd_tri_only": (10, {"s": [4, 2], "ep": 2, "p": [0.5]}, 32, 5),
    "logdet_like": (20, {"z": 2, "l": 3, "s": [6], "ep": 3}, 32, 3),
    "row1_n40": (40, {"z": 3, "l": 6, "q": [5], "s": [5], "ep": 3, "p": [0.4]}, 24, 11),
    "row2_n80": (80, {"z": 4, "l": 10, "q": [11, 11], "s": [8, 5], "ep": 6, "p": [0.4, 0.4]}, 24, 7),
}
# the row of CE_NS_VARIANTS and the footprint the plan must give, from ns_layout with both counts passed (test_psd_tri_ns_layout_host.py)
PLAN = {"mix_small": (0, 5312), "mix_all": (0, 12480), "psd_tri_only": (0, 8936), "logdet_like": (0, 15488), "row1_n40": (1, 25248), "row2_n80": (2, 101360)}
_POINTS: dict = {}

plain_part, plain_rows, blocks = PK.plain_part, PK.plain_rows, PK.blocks


def psd_rows(cones):
    return sum(k * (k + 1) // 2 for k in cones.get("s", []))


def ntri(cones):
    return cones.get("ep", 0) + len(cones.get("p", []))


def m_of(cones):
    return plain_rows(cones) + psd_rows(cones) + 3 * ntri(cones)


def triples(cones):
    """[(first row, None for an exponential triple | the power entry a)] in row order, behind the PSD blocks"""
    o = plain_rows(cones) + psd_rows(cones)
    out = [(o + 3 * k, None) for k in range(cones.get("ep", 0))]
    o += 3 * cones.get("ep", 0)
    return out + [(o + 3 * k, float(a)) for k, a in enumerate(cones.get("p", []))]


def proj(v, cones):
    """projection of one v onto the dual cone and its derivative D (module docstring)"""
    from oracle import oracle
    from test_gpu_refine import _proj
    o = plain_rows(cones)
    m = v.size
    out = v.copy(); D = np.zeros((m, m))
    out[:o], D[:o, :o] = _proj(v[:o], plain_part(cones))
    for r0, k in blocks(cones):
        d = k * (k + 1) // 2
        U, lam, Q, Bv = PK.block_eig(v[r0:r0 + d], k)
        out[r0:r0 + d] = PK.svec((U * np.maximum(lam, 0.0)) @ U.T)
        D[r0:r0 + d, r0:r0 + d] = (Q * Bv) @ Q.T
    for r0, a in triples(cones):
        w = v[r0:r0 + 3]
        if a is None:
            out[r0:r0 + 3] = oracle.proj_exp(w, dual=True); D[r0:r0 + 3, r0:r0 + 3] = oracle.dproj_exp(w, dual=True)
        else:
            out[r0:r0 + 3] = oracle.proj_pow(w, a, dual=True); D[r0:r0 + 3, r0:r0 + 3] = oracle.dproj_pow(w, a, dual=True)
    return out, D


def triple_eigs(D, cones):
    """per triple the eigenvalues of its block of D, ascending -- D = I: (1, 1, 1); D = 0: (0, 0, 0); boundary: (0, lambda, 1)"""
    return np.array([np.linalg.eigvalsh(0.5 * (D[r0:r0 + 3, r0:r0 + 3] + D[r0:r0 + 3, r0:r0 + 3].T)) for r0, _ in triples(cones)])


def state_counts(name):
    """over the shape's instances: (blocks with D = I, D = 0, mixed), (triples with D = I, D = 0, boundary), the smallest min(B, 1 - B) of a weighted PSD row, the
    smallest min(lambda, 1 - lambda) of a triple's weighted row (the kernel's snap at 1e-9 decides what is weighted), the largest weighted-row count"""
    _, cones, _, _, _, ref = problem(name)
    bc, tc, bm, tm, kw = [0, 0, 0], [0, 0, 0], 1.0, 1.0, 0
    for i in range(ref["x"].shape[0]):
        v = ref["y"][i] - ref["s"][i]
        kinds, mg = PK.block_states(v, cones)
        for k in kinds:
            bc[k] += 1
        bm = min(bm, mg)
        nw = 0
        for r0, k in blocks(cones):
            Bv = PK.block_eig(v[r0:r0 + k * (k + 1) // 2], k)[3]
            nw += int(((Bv != 0.0) & (Bv != 1.0)).sum())
        _, D = proj(v, cones)
        for ev in triple_eigs(D, cones):
            mix = ev[(ev >= 1e-9) & (ev <= 1 - 1e-9)]
            nw += mix.size
            tc[0 if (ev > 1 - 1e-9).all() else (1 if (ev < 1e-9).all() else 2)] += 1
            if mix.size:
                tm = min(tm, float(np.minimum(mix, 1 - mix).min()))
        kw = max(kw, nw)
    return tuple(bc), tuple(tc), bm, tm, kw


def residual(A, b, c, x, v, cones):
    """(F_x, F_y, y-hat, D) of one instance at (x, v)"""
    yh, D = proj(v, cones)
    return A.T @ yh + c, A @ x + (yh - v) - b, yh, D


kkt_matrix = PK.kkt_matrix


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


def dense_newton(A, b, c, x, v, cones):
    """(dx, dv, well conditioned) of one Newton step on the KKT residual of every instance"""
    B, m, n = A.shape
    dx = np.zeros((B, n)); dv = np.zeros((B, m)); ok = np.zeros(B, bool)
    for i in range(B):
        fx, fy, yh, D = residual(A[i], b[i], c[i], x[i], v[i], cones)
        J = kkt_matrix(A[i], D)
        if not np.isfinite(J).all() or np.linalg.cond(J) > 1e11:
            continue
        d = np.linalg.solve(J, -np.concatenate([fx, fy]))
        ok[i] = True; dx[i], dv[i] = d[:n], d[n:]
    return dx, dv, ok


rho = PK.rho


def problem(name):
    """(n, cones, A, b, c, the oracle's solution at eps 1e-10) of a shape: computed once, shared, not changed"""
    if name not in _POINTS:
        from oracle import oracle
        n, cones, B, seed = SHAPES[name]
        A, b, c = P.generate(n, cones, B, seed=seed)
        _POINTS[name] = (n, cones, A, b, c, oracle.solve_batch(A, b, c, cones, eps=1e-10, max_iters=200000))
    return _POINTS[name]


# ---------------------------------------------------------------------------------------------- the layout and the plan on the host (g++, no GPU)
HOST_SRC = r'''
#include <cstdio>
#include "ce_plan.h"
extern "C" {
// the kernel's carve (ce_backward_ns.h, TRI and PSD), restated with integer offsets: doubles from sm, then ints from (int *)sm, then the triples' doubles, then
// the blocks'.  out: first byte of Wt, lamt, psdU, psdEv, lamp, psdScr, psdXW, end of the carve
void h_carve_mixed(int n, int m, int nq, int ntri, int ns, int maxs, int psdrows, int NTILE, int NTHR, long *out) {
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
    out[0] = 8 * q; q += 9L * ntri;
    out[1] = 8 * q; q += 3L * ntri;
    ip = 2 * q;                      // (TRI && PSD: ip = (int *)(lamt + 3 ntri))
    ip += ip & 1;
    q = ip / 2;
    out[2] = 8 * q; q += (long)ns * maxs * maxs;
    out[3] = 8 * q; q += (long)ns * maxs;
    out[4] = 8 * q; q += psdrows;
    out[5] = 8 * q; q += 2L * maxs * maxs + 2 * maxs + 8;
    out[6] = 8 * q; q += 2L * NWB * maxs * maxs;
    out[7] = 8 * q;
}
// out: (first byte, byte count) of every segment of the mixed mode in the struct's order -- doubles, the union and its five members, ints, the triples' two
// segments, the five PSD segments -- then the first byte of slack and the footprint; returns the segment count
int h_layout_mixed(int n, int m, int nq, int ntri, int ns, int maxs, int psdrows, int NTILE, int NTHR, long *out) {
    const NsLayout L = ns_layout(n, m, nq, NTILE, NTHR, false, ntri, ns, maxs, psdrows);
    const NsSeg dbl[] = {L.A, L.vv, L.dv, L.rx, L.fvec, L.dB, L.cinfo, L.tvec, L.wgt, L.red, L.qaz, L.U, L.az, L.pub, L.Rbuf, L.qv2, L.mu};
    const NsSeg ints[] = {L.rkind, L.eqrow, L.ckind, L.ceq, L.cbase, L.erow, L.pcol, L.cmap, L.fcol, L.wrow, L.wsrc, L.wcnt, L.misc};
    const NsSeg top[] = {L.Wt, L.lamt, L.psdU, L.psdEv, L.lamp, L.psdScr, L.psdXW};
    int k = 0;
    for (const NsSeg &s : dbl) { out[2 * k] = 8L * s.off; out[2 * k + 1] = 8L * s.len; k++; }
    for (const NsSeg &s : ints) { out[2 * k] = 4L * s.off; out[2 * k + 1] = 4L * s.len; k++; }
    for (const NsSeg &s : top) { out[2 * k] = 8L * s.off; out[2 * k + 1] = 8L * s.len; k++; }
    out[2 * k] = 4L * L.slack.off; out[2 * k + 1] = (long)L.bytes;
    return k;
}
// out: the plain, QP, TRI (ntri triples) and PSD footprints -- the four older functions -- and the mixed one
void h_footprints5(int n, int m, int nq, int ntri, int ns, int maxs, int psdrows, int NTILE, int NTHR, long *out) {
    out[0] = (long)bwd_ns_lds_bytes_of(n, m, nq, NTILE, NTHR); out[1] = (long)bwd_ns_qp_lds_bytes_of(n, m, nq, NTILE, NTHR);
    out[2] = (long)bwd_ns_tri_lds_bytes_of(n, m, nq, ntri, NTILE, NTHR); out[3] = (long)bwd_ns_psd_lds_bytes_of(n, m, nq, ns, maxs, psdrows, NTILE, NTHR);
    out[4] = (long)bwd_ns_psd_tri_lds_bytes_of(n, m, nq, ntri, ns, maxs, psdrows, NTILE, NTHR);
}
void h_row(int v, int *ntile, int *nthr) { *ntile = NS_ROWS[v].NTILE; *nthr = NS_ROWS[v].NTHR; }
int h_rows() { return (int)std::size(NS_ROWS); }
// out: ns_variant, qp_ns_variant, tri_ns_variant, psd_ns_variant, psd_tri_ns_variant, psd_tri_ns_lds
int h_plan_mixed(const ce_template *tpl, long *out) {
    DevT T{}; std::vector<int> qoff, soff; CePlan P;
    plan_sizes(tpl, T, qoff, soff);
    const int rc = plan_engine(tpl, T, tpl->nnz_p, read_plan_env(), P);
    if (rc) return rc;
    out[0] = P.ns_variant; out[1] = P.qp_ns_variant; out[2] = P.tri_ns_variant; out[3] = P.psd_ns_variant; out[4] = P.psd_tri_ns_variant; out[5] = (long)P.psd_tri_ns_lds;
    return 0;
}
}
'''
HOST_PLAN_FIELDS = ("ns_variant", "qp_ns_variant", "tri_ns_variant", "psd_ns_variant", "psd_tri_ns_variant", "psd_tri_ns_lds")
PLAN_ENV = PK.PLAN_ENV
_HOST: dict = {}


def host_lib():
    """csrc/ce_plan.h and csrc/ce_ns_layout.h behind the shim above, compiled once per process with g++ into a temporary directory (as psd_ns_kit.host_lib)"""
    if "lib" not in _HOST:
        import ctypes as C
        import os
        import subprocess
        import tempfile
        from cvxpylayers_amd import _lib
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        _HOST["dir"] = tempfile.TemporaryDirectory(prefix="psd_tri_ns_host_")
        src, so = os.path.join(_HOST["dir"].name, "host.cpp"), os.path.join(_HOST["dir"].name, "libpsd_tri_ns_host.so")
        with open(src, "w") as f:
            f.write(HOST_SRC)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__host__=", "-D__device__=", "-shared", "-fPIC", "-I", os.path.join(root, "cvxpylayers_amd", "csrc"),
                               "-I", os.path.join(root, "include"), "-o", so, src])
        L = C.CDLL(so)
        L.h_carve_mixed.argtypes = [C.c_int] * 9 + [C.POINTER(C.c_long)]; L.h_carve_mixed.restype = None
        L.h_layout_mixed.argtypes = [C.c_int] * 9 + [C.POINTER(C.c_long)]
        L.h_footprints5.argtypes = [C.c_int] * 9 + [C.POINTER(C.c_long)]; L.h_footprints5.restype = None
        L.h_row.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.h_plan_mixed.argtypes = [C.POINTER(_lib.CeTemplate), C.POINTER(C.c_long)]
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
    return dict(zip(HOST_PLAN_FIELDS, out)) if host_lib().h_plan_mixed(C.byref(t), out) == 0 else None

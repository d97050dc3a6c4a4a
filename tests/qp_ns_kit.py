"""Shared by test_gpu_qp_jvp.py and test_gpu_qp_refine.py: the instances, structures and dense numpy references of the search-free elimination with a quadratic
objective (k_backward_ns<..., QP> behind ce_jvp_qp / ce_refine_qp).  Nothing here needs a GPU until an engine is asked for.

Instances: P.generate(n, cones, B, seed) with P_i = G G^T / n + 1/2 I, G = default_rng(seed + 1000).standard_normal((B, n, n)); rank = n / 2 draws a (B, n, n / 2)
G and leaves the 1/2 I out.  Dense references, per instance, in solver form (A x + s = b), v = y - s, D = DPi(v) on the dual cone:
    [[P, A^T D], [A, D - I]] (d_x, d_v) = -(g_x, g_y),   g_x = tP x + tA^T y + tc,   g_y = tA x - tb,   dx = d_x, dy = D d_v, ds = (D - I) d_v
and the same matrix with the KKT residual (F_x = P x + A^T y^ + c, F_y = A x + s^ - b) on the right for one Newton step."""
import numpy as np
import torch

from cvxpylayers_amd import problems as P
from test_gpu_refine import _proj
from test_quad_objective import _p_values, _upper_structure

# name -> (n, cones, B, seed): the shapes of the identity table the feature was specified with
SHAPES = {
    "equality_qp": (6, {"z": 2, "l": 0, "q": []}, 16, 1),
    "small_mixed": (12, {"z": 2, "l": 6, "q": [4, 5]}, 48, 1),
    "ragged_cones": (20, {"z": 3, "l": 10, "q": [3, 7, 2, 5, 1]}, 48, 4),
    "soc_only": (25, {"z": 0, "l": 0, "q": [6] * 6}, 32, 5),
    "metric": (P.CONFIGS["M"]["n"], P.CONFIGS["M"]["cones"], 48, 3),
    "row2_n80": (80, {"z": 0, "l": 10, "q": [11] * 8}, 24, 7),
    "square_equalities": (6, {"z": 6, "l": 0, "q": []}, 16, 2),          # p = n: nf = 0, nothing is left to sweep
}
RANK_HALF = ("metric", "small_mixed")


def full_structure(n):
    """dense CSC structure of an n x n matrix, both triangles"""
    return np.tile(np.arange(n), n).astype(np.int32), (np.arange(n + 1) * n).astype(np.int32), (n, n)


def quad_matrices(n, B, seed, rank=None):
    r = n if rank is None else rank
    G = np.random.default_rng(seed + 1000).standard_normal((B, n, r))
    Pm = G @ G.transpose(0, 2, 1) / n
    return Pm + 0.5 * np.eye(n) if rank is None else Pm


def instance(name, rank_half=False):
    n, cones, B, seed = SHAPES[name]
    A, b, c = P.generate(n, cones, B, seed=seed)
    return n, cones, A, b, c, quad_matrices(n, B, seed, n // 2 if rank_half else None)


def box_qp(nx=50, B=24):
    """the box QP of test_quad_objective.py::test_native_qp_kernels_match_the_oracle_on_box_qps (config-2 shape): (cones, A, b, c, P, template)"""
    rng = np.random.default_rng(0)
    Fm = rng.standard_normal((nx, nx)) / np.sqrt(nx); g = rng.standard_normal((B, nx))
    lo = -0.5 - 0.5 * rng.random((B, nx)); hi = 0.5 + 0.5 * rng.random((B, nx))
    Pn = np.broadcast_to(2 * Fm.T @ Fm, (B, nx, nx)).copy() * (1 + 0.1 * rng.random((B, 1, 1)))
    An = np.broadcast_to(np.concatenate([-np.eye(nx), np.eye(nx)], axis=0), (B, 2 * nx, nx)).copy()
    cones = {"z": 0, "l": 2 * nx, "q": []}
    return cones, An, np.concatenate([-lo, hi], axis=1), -2 * g @ Fm, Pn, P.dense_template(nx, cones, pattern=(An[0] != 0))


def inactive_box(n=10, B=16):
    """no active row at all: box rows +-I with bounds 100, P and c from default_rng(5) -- neq = 0 and H = 0, the reduced Hessian is P alone"""
    rng = np.random.default_rng(5)
    G = rng.standard_normal((B, n, n)); Pm = G @ G.transpose(0, 2, 1) / n + 0.5 * np.eye(n)
    c = rng.standard_normal((B, n))
    An = np.broadcast_to(np.concatenate([-np.eye(n), np.eye(n)], axis=0), (B, 2 * n, n)).copy()
    cones = {"z": 0, "l": 2 * n, "q": []}
    return cones, An, np.full((B, 2 * n), 100.0), c, Pm, P.dense_template(n, cones, pattern=(An[0] != 0))


def qp_engine(tpl, struct):
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
    return ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, torch.device("cuda", 0), p_structure=struct[:2])


def p_tangent_values(tP, struct):
    """(B, n, n) symmetric dense tangent -> (B, nnz_p) in the structure's order (a one-triangle entry stands for both matrix entries)"""
    return np.ascontiguousarray(_p_values(tP, struct))


def device_values(tpl, A, b, c, Pm, struct):
    """A_bm (B, nnz_aug), q_t (n + 1, B), P_bm (B, nnz_p) on the device"""
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    return (torch.from_numpy(A_eval).cuda().t().contiguous(), torch.from_numpy(q_eval).cuda(), torch.from_numpy(np.ascontiguousarray(_p_values(Pm, struct))).cuda())


def kkt_matrix(A, Pm, v, cones):
    m, n = A.shape
    _, D = _proj(v, cones)
    return np.block([[Pm, A.T @ D], [A, D - np.eye(m)]]), D


def dense_jvp(A, Pm, x, y, s, tA, tb, tc, tP, cones):
    """(dx, dy, ds, well conditioned) of every instance by a dense solve of the system in the module docstring; tangents may be None (zero)"""
    B, m, n = A.shape
    out = np.zeros((B, n)), np.zeros((B, m)), np.zeros((B, m)); ok = np.zeros(B, bool)
    for i in range(B):
        J, D = kkt_matrix(A[i], Pm[i], y[i] - s[i], cones)
        gx = np.zeros(n); gy = np.zeros(m)
        if tP is not None:
            gx += tP[i] @ x[i]
        if tA is not None:
            gx += tA[i].T @ y[i]; gy += tA[i] @ x[i]
        if tc is not None:
            gx += tc[i]
        if tb is not None:
            gy -= tb[i]
        if not np.isfinite(J).all() or np.linalg.cond(J) > 1e11:
            continue
        d = np.linalg.solve(J, -np.concatenate([gx, gy]))
        ok[i] = True
        out[0][i] = d[:n]; out[1][i] = D @ d[n:]; out[2][i] = (D - np.eye(m)) @ d[n:]
    return out + (ok,)


def qp_residual(A, b, c, Pm, x, v, cones):
    yh, D = _proj(v, cones)
    return Pm @ x + A.T @ yh + c, A @ x + (yh - v) - b, yh, D


def qp_rho(A, b, c, Pm, x, y, s):
    """rho of every instance at the arrays as given (include/cone_engine.h ce_refine with F_x = P x + A^T y + c), in extended precision"""
    L = np.longdouble
    A, b, c, Pm, x, y, s = (np.asarray(t, dtype=L) for t in (A, b, c, Pm, x, y, s))
    fx = np.einsum("bij,bj->bi", Pm, x) + np.einsum("bij,bi->bj", A, y) + c; fy = np.einsum("bij,bj->bi", A, x) + s - b
    num = np.maximum(np.abs(fx).max(axis=1), np.abs(fy).max(axis=1))
    return (num / (1 + np.maximum(np.abs(b).max(axis=1), np.abs(c).max(axis=1)))).astype(np.float64)


def sym_tangent(B, n, seed):
    T = np.random.default_rng(seed).standard_normal((B, n, n))
    return 0.5 * (T + T.transpose(0, 2, 1))

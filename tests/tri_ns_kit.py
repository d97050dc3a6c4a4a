"""Shared by test_gpu_tri_jvp.py, test_gpu_tri_refine.py and test_tri_ns_layout_host.py: the shapes, instances and dense numpy references of the search-free
elimination with exponential / power triples (k_backward_ns<..., TRI> behind ce_jvp / ce_refine).  Nothing here needs a GPU until an engine is asked for.

Instances: P.generate(n, cones, B, seed) at the oracle's point (eps 1e-10, max_iters 200 000).  Dense references, per instance, in solver form (A x + s = b),
v = y - s, D = DPi(v) on the dual cone -- test_gpu_refine._proj for the zero / nonnegative / second-order rows, the oracle's dproj_exp / dproj_pow (dual=True) for
the triples:
    [[0, A^T D], [A, D - I]] (d_x, d_v) = -(g_x, g_y),   g_x = tA^T y + tc,   g_y = tA x - tb,   dx = d_x, dy = D d_v, ds = (D - I) d_v
and the same matrix with the KKT residual (F_x = A^T y^ + c, F_y = A x + s^ - b) on the right for one Newton step (qp_ns_kit.py with P = 0)."""
import numpy as np

from cvxpylayers_amd import problems as P

# name -> (n, cones, B, seed, expected row of CE_NS_VARIANTS)
SHAPES = {
    "exp_small": (6, {"z": 1, "l": 3, "q": [], "ep": 2}, 16, 1, 0),
    "exp_pow_mixed": (12, {"z": 2, "l": 6, "q": [4], "ep": 2, "p": [0.3, -0.6]}, 48, 1, 0),
    "triples_only": (9, {"z": 0, "l": 0, "q": [], "ep": 3, "p": [0.5, 0.25]}, 32, 5, 0),
    "E": (P.CONFIGS["E"]["n"], P.CONFIGS["E"]["cones"], 48, 3, 1),
    "row2_n80": (80, {"z": 4, "l": 20, "q": [11] * 4, "ep": 12, "p": [0.4] * 4}, 24, 7, 2),
}
_POINTS: dict = {}


def plain_part(cones):
    return {"z": cones.get("z", 0), "l": cones.get("l", 0), "q": list(cones.get("q", []))}


def plain_rows(cones):
    return cones.get("z", 0) + cones.get("l", 0) + sum(cones.get("q", []))


def triples(cones):
    """[(first row, None for an exponential triple | the power entry a)] in row order (z, l, q, ep, p; no PSD block in these templates)"""
    o = plain_rows(cones)
    out = [(o + 3 * k, None) for k in range(cones.get("ep", 0))]
    o += 3 * cones.get("ep", 0)
    return out + [(o + 3 * k, float(a)) for k, a in enumerate(cones.get("p", []))]


def proj(v, cones, ld=False):
    """projection of one v onto the dual cone and its derivative D: the plain rows by test_gpu_refine._proj, the triples by the oracle (dual=True)"""
    from oracle import oracle
    from test_gpu_refine import _proj
    o = plain_rows(cones)
    m = v.size
    out = v.copy(); D = np.zeros((m, m))
    out[:o], D[:o, :o] = _proj(v[:o], plain_part(cones))
    for r0, a in triples(cones):
        w = v[r0:r0 + 3]
        if a is None:
            out[r0:r0 + 3] = oracle.proj_exp(w, dual=True); D[r0:r0 + 3, r0:r0 + 3] = oracle.dproj_exp(w, dual=True)
        else:
            out[r0:r0 + 3] = oracle.proj_pow(w, a, dual=True); D[r0:r0 + 3, r0:r0 + 3] = oracle.dproj_pow(w, a, dual=True)
    return out, D


def triple_states(v, cones):
    """per triple of one v: the eigenvalues of D (ascending) -- D = I: (1, 1, 1); D = 0: (0, 0, 0); boundary: (0, lambda, 1)"""
    _, D = proj(v, cones)
    return np.array([np.linalg.eigvalsh(0.5 * (D[r0:r0 + 3, r0:r0 + 3] + D[r0:r0 + 3, r0:r0 + 3].T)) for r0, _ in triples(cones)])


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
    solve in extended precision (the reference of the bounds that are ten times the reference's own distance)"""
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
        n, cones, B, seed, _ = SHAPES[name]
        A, b, c = P.generate(n, cones, B, seed=seed)
        _POINTS[name] = (n, cones, A, b, c, oracle.solve_batch(A, b, c, cones, eps=1e-10, max_iters=200000))
    return _POINTS[name]

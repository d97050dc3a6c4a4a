"""Shared by test_lpgd_host.py, test_gpu_lpgd_kernels.py and test_gpu_lpgd.py: LPGD (Lagrangian proximal gradient descent, Paulus et al. 2024) stated in numpy on
top of the oracle as it stands -- oracle.solve_batch on perturbed data plus the formulas of DESIGN.md section 3.11.  Nothing here needs a GPU.

Canonical program  min c^T x + 1/2 x^T P x  s.t.  A x + s = b, s in K;   L(x, y; theta) = c^T x + 1/2 x^T P x + y^T (A x - b).
For cotangents dx, dy, a step tau > 0 and a proximal weight rho >= 0 the program perturbed at +tau has
    c+ = c + tau dx - rho x*,   b+ = b - tau dy,   P+ = P + rho I,   A unchanged               (-tau: the same with tau -> -tau),
and with G = dL/dtheta  (G_A = y x^T, G_b = -y, G_c = x, G_P = 1/2 x x^T in solver form)
    lpgd_right = [G(+) - G(*)] / tau,   lpgd_left = [G(*) - G(-)] / tau,   lpgd = [G(+) - G(-)] / (2 tau).
Products are differenced in the staged form  y_b x_b^T - y_a x_a^T = y_b Dx^T + Dy x_a^T  (Dx = x_b - x_a, Dy = y_b - y_a), as the kernel does.

The derived bound of the comparisons.  G is bilinear in the point, so an error e_a, e_b (max norm over x and y) in the two points moves an entry of the
differenced gradient by at most (|x|_inf + |y|_inf + 1) (e_a + e_b) / delta up to second order in e: the bound of the issue,
    (|x|_inf + |y|_inf + 1) (delta_0 + delta_tau) / tau.
Against the ADJOINT on a fixed active set of a QP the points move linearly in tau, x(+-tau) = x* +- tau x', y(+-tau) = y* +- tau y': the central difference of
y x^T is then exactly the adjoint's y* x'^T + y' x*^T, the one-sided ones carry the second-order term tau y' x'^T = Dy Dx^T / tau on top -- for dA and dP only
(G_b and G_c are linear in the point).  It shrinks with tau while the bound grows as 1 / tau: test_lpgd_host.py picks tau so that it lies below the bound.
"""
from __future__ import annotations

import numpy as np

MODES = ("lpgd", "lpgd_left", "lpgd_right")
SOC_SHAPE = (12, {"z": 2, "l": 6, "q": [4, 5]})


def sides(mode):
    return {"lpgd": (1.0, -1.0), "lpgd_left": (-1.0,), "lpgd_right": (1.0,)}[mode]


def perturbed_data(b, c, P, x0, dx, dy, tau, rho):
    """(b_t, c_t, P_t) of the program perturbed by the signed step tau"""
    n = c.shape[1]
    c_t = c + tau * dx - rho * x0
    b_t = b - tau * dy if dy is not None else b
    P_t = P
    if rho != 0.0:
        P_t = (np.zeros((c.shape[0], n, n)) if P is None else np.array(P, dtype=np.float64)) + rho * np.eye(n)[None]
    return b_t, c_t, P_t


def diff_G(pa, pb, delta, with_P=False):
    """[G(pb) - G(pa)] / delta in the staged form; points are (x, y).  Returns dict(dA (B,m,n), db, dc[, dP (B,n,n)]) in solver form, and `scale`, the sum of the
    absolute values of the two staged terms of dA (for rounding bounds)."""
    (xa, ya), (xb, yb) = pa, pb
    Dx, Dy = xb - xa, yb - ya
    t1, t2 = yb[:, :, None] * Dx[:, None, :], Dy[:, :, None] * xa[:, None, :]
    out = dict(dA=(t1 + t2) / delta, db=-Dy / delta, dc=Dx / delta, scale=(np.abs(t1) + np.abs(t2)) / delta)
    if with_P:
        out["dP"] = 0.5 * (xb[:, :, None] * Dx[:, None, :] + Dx[:, :, None] * xa[:, None, :]) / delta
    return out


def oracle_points(A, b, c, cones, dx, dy, tau, rho, mode, P=None, base=None, **opts):
    """the base point (solved here unless given) and the perturbed points of `mode`, all by oracle.solve_batch warm-started at the base point:
    dict(base=ref, pts={sign: ref})"""
    from oracle import oracle
    if base is None:
        base = oracle.solve_batch(A, b, c, cones, P=P, **opts)
    pts = {}
    for sg in sides(mode):
        b_t, c_t, P_t = perturbed_data(b, c, P, base["x"], dx, dy, sg * tau, rho)
        pts[sg] = oracle.solve_batch(A, b_t, c_t, cones, P=P_t, warm=(base["x"], base["y"], base["s"]), **opts)
    return dict(base=base, pts=pts)


def combine(mode, tau, base, pts, with_P=False):
    """the three modes from points given as (x, y) pairs"""
    if mode == "lpgd_right":
        return diff_G(base, pts[1.0], tau, with_P)
    if mode == "lpgd_left":
        return diff_G(pts[-1.0], base, tau, with_P)
    return diff_G(pts[-1.0], pts[1.0], 2.0 * tau, with_P)


def oracle_lpgd(A, b, c, cones, dx, dy, tau, rho, mode, P=None, base=None, **opts):
    """oracle LPGD: gradients dict(dA, db, dc[, dP]) plus the points they were formed from (`points`)"""
    r = oracle_points(A, b, c, cones, dx, dy, tau, rho, mode, P=P, base=base, **opts)
    xy = lambda ref: (ref["x"], ref["y"])
    out = combine(mode, tau, xy(r["base"]), {k: xy(v) for k, v in r["pts"].items()}, with_P=P is not None)
    out["points"] = r
    return out


def point_bound(x, y, d0, dtau, tau):
    """(|x|_inf + |y|_inf + 1) (delta_0 + delta_tau) / tau per instance"""
    return (np.abs(x).max(axis=1) + np.abs(y).max(axis=1) + 1.0) * (d0 + dtau) / tau


def to_boundary(tpl, g):
    """solver-form gradients -> the boundary convention A_eval = [-A.data, b], q_eval = [c, d]: dA_eval (nnz_aug, B), dq_eval (n+1, B)"""
    rows = np.asarray(tpl.indices)
    cols = np.repeat(np.arange(tpl.n + 1), np.diff(tpl.indptr))
    B = g["dc"].shape[0]
    aug = np.concatenate([-g["dA"], g["db"][:, :, None]], axis=2)
    return aug[:, rows, cols].T.copy(), np.concatenate([g["dc"].T, np.zeros((1, B))], axis=0)


def cone_class(v, cones):
    """the face of K* (x) K each block of v = y - s lies on: per instance a tuple -- sign of every zero / nonnegative row, and for every second-order block
    0 (inside -K), 1 (inside K), 2 (outside both): LPGD and the adjoint agree to first order only while this does not change between the points compared"""
    z, l, qs = int(cones.get("z", 0)), int(cones.get("l", 0)), [int(k) for k in cones.get("q", [])]
    out = [np.sign(v[:, z:z + l]).astype(int)]
    off = z + l
    for k in qs:
        t, nr = v[:, off], np.linalg.norm(v[:, off + 1:off + k], axis=1)
        out.append(np.where(nr <= t, 1, np.where(nr <= -t, 0, 2))[:, None])
        off += k
    return np.concatenate(out, axis=1)


LAYER_CASES = ("soc", "psd", "exp", "qp_native", "shared_a")
LAYER_TAU = 0.05


def layer_case(name):
    """The shapes of the layer tests (B <= 70): dict(tpl, A, b, c, cones, P (B, n, n) or None, struct (CSC, upper triangle) or None, dx, dy, shared).  dy is zero
    on the rows without a b slot in the template (the perturbation b - tau dy has no slot to travel in there: test_gpu_lpgd.py checks that case on its own)."""
    from cvxpylayers_amd import problems as P
    Pm = struct = None
    shared = False
    if name in ("soc", "psd", "exp"):
        n, cones, B, seed = {"soc": (*SOC_SHAPE, 16, 2), "psd": (4, {"z": 1, "l": 0, "q": [], "s": [3]}, 8, 0), "exp": (5, {"z": 0, "l": 4, "q": [], "s": [], "ep": 2}, 8, 3)}[name]
        A, b, c = P.generate(n, cones, B, seed=seed)
        tpl = P.dense_template(n, cones)
    elif name == "qp_native":
        nx, B, seed = 6, 16, 0
        A1, b, c, P1, struct, _ = P.native_box_qp_batch(nx, B, seed=seed)
        cones = {"z": 0, "l": 2 * nx, "q": []}
        A, Pm = np.broadcast_to(A1, (B,) + A1.shape).copy(), np.broadcast_to(P1, (B, nx, nx)).copy()
        tpl = P.dense_template(nx, cones, pattern=(A1 != 0))
    else:
        B, seed, shared = 6, 0, True
        A1, b1, c, cones, tpl = P.portfolio_c5_batch(B, nw=60, kf=9)
        A, b = np.broadcast_to(A1, (B,) + A1.shape).copy(), np.broadcast_to(b1, (B, len(b1))).copy()
    rng = np.random.default_rng(seed + 100)
    dx, dy = rng.standard_normal((B, tpl.n)), rng.standard_normal((B, tpl.m))
    has_slot = np.zeros(tpl.m, bool)
    has_slot[np.asarray(tpl.indices)[tpl.indptr[tpl.n]:tpl.indptr[tpl.n + 1]]] = True
    return dict(tpl=tpl, A=A, b=b, c=c, cones=cones, P=Pm, struct=struct, dx=dx, dy=dy * has_slot[None], shared=shared)


def simplex_projection(v):
    """Euclidean projection of the rows of v onto {x >= 0, 1^T x = 1} (sort-based closed form)"""
    u = -np.sort(-v, axis=1)
    css = np.cumsum(u, axis=1) - 1.0
    k = np.arange(1, v.shape[1] + 1)
    cond = u - css / k > 0
    rho = cond.shape[1] - 1 - np.argmax(cond[:, ::-1], axis=1)
    theta = css[np.arange(v.shape[0]), rho] / (rho + 1)
    return np.maximum(v - theta[:, None], 0.0)


def simplex_program(n, B):
    """min c^T x over {x >= 0, 1^T x = 1} in solver form: row 0 the equality, rows 1..n the nonnegativity; returns (A (B,m,n), b (B,m), cones)"""
    A = np.zeros((1 + n, n)); A[0] = 1.0; A[1:] = -np.eye(n)
    b = np.zeros(1 + n); b[0] = 1.0
    return np.broadcast_to(A, (B, 1 + n, n)).copy(), np.broadcast_to(b, (B, 1 + n)).copy(), {"z": 1, "l": n, "q": []}


def simplex_draw(n, B, tau, seed, gap=0.05):
    """c, dx (B, n) by seeded rejection: the two smallest entries of c, of c + tau dx and of c - tau dx are each at least `gap` apart"""
    rng = np.random.default_rng(seed)
    cs, ds = [], []
    while len(cs) < B:
        c, d = rng.standard_normal(n), rng.standard_normal(n) * (0.5 / tau)
        if all(np.diff(np.sort(v)[:2])[0] >= gap for v in (c, c + tau * d, c - tau * d)):
            cs.append(c); ds.append(d)
    return np.array(cs), np.array(ds)

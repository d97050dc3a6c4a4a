"""Planted KKT points for the search-free elimination at the edges of its plan (tests/test_ns_edge_kit.py, tests/test_gpu_ns_mode_edges.py).  Host only.

The forward derivative, the adjoint and a Newton step are linear systems AT a point, so the point is planted instead of solved for (the oracle does not converge on
the tall templates at the LDS edges): draw A = N(0, 1) / sqrt(n), x and v; set y = Pi_K*(v), s = y - v (exactly complementary), b = A x + s and c = -A^T y
(QP kind: c = -(P x + A^T y), P from qp_ns_kit.quad_matrices).  (x, y, s) is then a KKT point to rounding, at any size.

v per block: zero rows Gaussian; nonnegative rows |v| >= 0.1; a second-order block in a chosen state -- "in" (inside the dual cone, D = I), "out" (inside the
polar cone, D = 0), "bd" (D general, t = |u| U(-0.6, 0.6)); triples Gaussian, redrawn only when the instance cannot take another unit eigenvalue.

Regularity.  With D = sum of projectors, J = [[P, A^T D], [A, D - I]] reduces to [[P + H, A_1^T], [A_1, 0]] in dx: A_1 the k1 directions of unit eigenvalue (zero
rows, active nonnegative rows, the rows of an "in" block, one direction per "bd" block or boundary triple), H = sum over the L directions with an eigenvalue in (0, 1)
(d - 2 per "bd" block of dimension d, one per boundary triple).  With P = 0 it is nonsingular iff k1 <= n <= k1 + L (generically); random v has k1 > n at the tall
shapes and is singular.  The kit keeps nf = n - k1 = min(ceil(L / 2), n - k1 without nonnegative rows) free directions -- the reduced Hessian the kernel sweeps is
then not empty wherever the cones give it an entry -- and makes exactly n - nf - (the other unit directions) nonnegative rows active.  QP kind: P is positive
definite, any k1 <= n is regular; half of the remaining directions are made active rows.  tests/test_ns_edge_kit.py asserts the outcome on every instance of every
shape the GPU test uses: J finite, cond(J) <= 1e11, KKT residual <= 1e-13 (1 + max(|b|, |c|))."""
import numpy as np

import plan_kit as pk
from cvxpylayers_amd import problems as P

EIG_SNAP = 1e-9          # an eigenvalue of a triple's D within this of 0 / 1 counts as 0 / 1 (tri_ns_kit's rule in its tests)
_POINTS: dict = {}


def batch_of(shape):
    n, m = shape[1], P.cone_rows(shape[2])
    return 24 if n * m <= 6000 else 8


def project(v, cones):
    """y = Pi_K*(v) of every instance: zero rows free, nonnegative rows, second-order blocks; the triples by the oracle (dual=True)"""
    import tri_ns_kit as TK
    z, l = cones.get("z", 0), cones.get("l", 0)
    y = v.copy()
    y[:, z:z + l] = np.maximum(v[:, z:z + l], 0.0)
    o = z + l
    for d in cones.get("q", []):
        t, w = v[:, o], v[:, o + 1:o + d]
        nz = np.linalg.norm(w, axis=1)
        if d == 1:
            y[:, o] = np.maximum(t, 0.0)
        else:
            a = np.where(nz <= t, 1.0, np.where(nz <= -t, 0.0, (t + nz) / (2 * np.where(nz > 0, nz, 1.0))))
            inside = nz <= t
            y[:, o] = np.where(inside, t, a * nz)
            y[:, o + 1:o + d] = np.where(inside[:, None], w, a[:, None] * w)
        o += d
    if TK.triples(cones):
        from oracle import oracle
        for i in range(v.shape[0]):
            for r0, a in TK.triples(cones):
                y[i, r0:r0 + 3] = oracle.proj_exp(v[i, r0:r0 + 3], dual=True) if a is None else oracle.proj_pow(v[i, r0:r0 + 3], a, dual=True)
    return y


def _triple_eigs(w, a):
    from oracle import oracle
    D = oracle.dproj_exp(w, dual=True) if a is None else oracle.dproj_pow(w, a, dual=True)
    e = np.linalg.eigvalsh(0.5 * (D + D.T))
    mid = e[(e > EIG_SNAP) & (e < 1 - EIG_SNAP)]
    return int((e > 1 - EIG_SNAP).sum()), int(mid.size), float(np.minimum(mid, 1 - mid).min()) if mid.size else 1.0


def plant(shape, B=None, seed=0, active=None, extra_units=0, extra_L=0, triple_kinds=None, triple_margin=0.0):
    """The planted batch of a shape (kind, n, cones, states): dict with A, b, c, x, y, s, v, Pm (QP kind, else None), cones, kind, n, m, and per instance k1 (unit
    directions), L (directions with an eigenvalue in (0, 1)), nf.  active: the number of active nonnegative rows, instead of the rule of the module docstring.
    extra_units, extra_L: unit and interior directions of cones the caller plants itself (psd_edge_kit: the PSD blocks), counted by the rule and in k1, L.
    triple_kinds: the (unit, interior) eigenvalue counts a triple may be drawn with, beside the room rule (None: any); triple_margin: the least distance of a
    triple's interior eigenvalue from 0 and 1."""
    import tri_ns_kit as TK
    kind, n, cones, states = shape
    m = P.cone_rows(cones)
    B = batch_of(shape) if B is None else B
    z, l, q = cones.get("z", 0), cones.get("l", 0), list(cones.get("q", []))
    assert len(states) == len(q), shape
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((B, m, n)) / np.sqrt(n)
    x = rng.standard_normal((B, n))
    v = np.zeros((B, m))
    v[:, :z] = rng.standard_normal((B, z))
    units = np.full(B, z + extra_units); L = np.full(B, extra_L)
    o = z + l
    for d, st in zip(q, states):
        u = rng.standard_normal((B, d - 1)); nu = np.linalg.norm(u, axis=1)
        far = nu * (1.2 + rng.random(B)) + 0.1 + np.abs(rng.standard_normal(B))
        if st == "in":
            t = far; units = units + d
        elif st == "out":
            t = -far
        else:
            assert st == "bd" and d >= 2, shape
            t = nu * rng.uniform(-0.6, 0.6, B); units = units + 1; L = L + (d - 2)
        v[:, o] = t; v[:, o + 1:o + d] = u
        o += d
    seen = np.zeros(3, int)          # triples with D = I, D = 0, on the boundary
    for i in range(B):
        room = max(0, (n - units[i]) // 2)          # unit directions the triples of this instance may take
        for r0, a in TK.triples(cones):
            for attempt in range(400):
                w = rng.standard_normal(3)
                k, mid, margin = _triple_eigs(w, a)
                if k <= room and margin >= triple_margin and (triple_kinds is None or (k, mid) in triple_kinds):
                    break
            else:
                raise AssertionError(f"no triple state with at most {room} unit eigenvalues in 400 draws: {shape}")
            v[i, r0:r0 + 3] = w; room -= k; units[i] += k; L[i] += mid
            seen[0 if k == 3 else 1 if k == 0 and mid == 0 else 2] += 1
    if (units > n).any():
        raise AssertionError(f"more unit directions than variables without a nonnegative row: {shape} {units}")
    if active is not None:
        act = np.full(B, active)
    elif kind == "qp":
        act = np.minimum(l, (n - units) // 2)
    else:
        act = n - np.minimum((L + 1) // 2, n - units) - units
    if (act < 0).any() or (act > l).any():
        raise AssertionError(f"{shape}: {act} active nonnegative rows asked of {l}")
    mag = 0.1 + np.abs(rng.standard_normal((B, l)))
    for i in range(B):
        sign = -np.ones(l); sign[rng.permutation(l)[:act[i]]] = 1.0
        v[i, z:z + l] = sign * mag[i]
    k1 = units + act
    y = project(v, cones); s = y - v
    Pm = None
    if kind == "qp":
        import qp_ns_kit as QK
        Pm = QK.quad_matrices(n, B, seed)
    b = np.einsum("bij,bj->bi", A, x) + s
    c = -np.einsum("bij,bi->bj", A, y) - (np.einsum("bij,bj->bi", Pm, x) if Pm is not None else 0.0)
    return dict(shape=shape, kind=kind, n=n, m=m, cones=cones, A=A, b=b, c=c, x=x, y=y, s=s, v=v, Pm=Pm, k1=k1, L=L, nf=n - k1, triple_states=seen, seed=seed)


def regularity(pt):
    """(condition of J, KKT residual relative to 1 + max(|b|, |c|)) of every instance, with D and y-hat from the references' own projection (tri_ns_kit.proj):
    independent of project() above.  Cached in the point."""
    if "cond" not in pt:
        import tri_ns_kit as TK
        B, n, m = pt["x"].shape[0], pt["n"], pt["m"]
        cond = np.zeros(B); res = np.zeros(B)
        for i in range(B):
            yh, D = TK.proj(pt["v"][i], pt["cones"])
            Pi = pt["Pm"][i] if pt["Pm"] is not None else np.zeros((n, n))
            J = np.block([[Pi, pt["A"][i].T @ D], [pt["A"][i], D - np.eye(m)]])
            cond[i] = np.linalg.cond(J) if np.isfinite(J).all() else np.inf
            fx = Pi @ pt["x"][i] + pt["A"][i].T @ yh + pt["c"][i]; fy = pt["A"][i] @ pt["x"][i] + (yh - pt["v"][i]) - pt["b"][i]
            res[i] = max(np.abs(fx).max(), np.abs(fy).max()) / (1 + max(np.abs(pt["b"][i]).max(), np.abs(pt["c"][i]).max()))
        pt["cond"], pt["resid"] = cond, res
    return pt["cond"], pt["resid"]


def tangents(pt, seed=1):
    """(tA, tb, tc, tP or None): Gaussian; tP symmetric (QP kind)"""
    rng = np.random.default_rng(pt["seed"] + 7919 * seed)
    B, n, m = pt["x"].shape[0], pt["n"], pt["m"]
    tA, tb, tc = rng.standard_normal((B, m, n)), rng.standard_normal((B, m)), rng.standard_normal((B, n))
    tP = None
    if pt["kind"] == "qp":
        T = rng.standard_normal((B, n, n)); tP = 0.5 * (T + T.transpose(0, 2, 1))
    return tA, tb, tc, tP


def dense_jvp(pt, t):
    """(dx, dy, ds, well conditioned) of the planted batch: tri_ns_kit.dense_jvp (P = 0) or qp_ns_kit.dense_jvp"""
    tA, tb, tc, tP = t
    if pt["kind"] == "qp":
        import qp_ns_kit as QK
        return QK.dense_jvp(pt["A"], pt["Pm"], pt["x"], pt["y"], pt["s"], tA, tb, tc, tP, pt["cones"])
    import tri_ns_kit as TK
    return TK.dense_jvp(pt["A"], pt["x"], pt["y"], pt["s"], tA, tb, tc, pt["cones"])[:4]


def perturbed(pt, rel=1e-6, seed=2):
    """(x', y', s', v'): every entry of the planted (x, v) moved by rel * N(0, 1) clipped to 3, relative to itself -- far inside the 0.1 margins of the rows and the
    0.4 |u| of the blocks, so that the active set is the planted one; y' = Pi_K*(v'), s' = y' - v'"""
    rng = np.random.default_rng(pt["seed"] + 7919 * seed)
    x1 = pt["x"] * (1 + rel * np.clip(rng.standard_normal(pt["x"].shape), -3, 3))
    v1 = pt["v"] * (1 + rel * np.clip(rng.standard_normal(pt["v"].shape), -3, 3))
    y1 = project(v1, pt["cones"])
    return x1, y1, y1 - v1, v1


def dense_newton(pt, x1, v1):
    """(x, v) after one extended-precision dense Newton step from (x1, v1), and the well-conditioned flags"""
    if pt["kind"] == "qp":
        dx, dv, ok = qp_dense_newton(pt["A"], pt["b"], pt["c"], pt["Pm"], x1, v1, pt["cones"])
    else:
        import tri_ns_kit as TK
        dx, dv, ok = TK.dense_newton(pt["A"], pt["b"], pt["c"], x1, v1, pt["cones"], longdouble=True)
    return x1 + dx, v1 + dv, ok


def qp_dense_newton(A, b, c, Pm, x, v, cones):
    """tri_ns_kit.dense_newton(..., longdouble=True) with P: the residual and one step of iterative refinement of the solve in extended precision"""
    import qp_ns_kit as QK
    B, m, n = A.shape
    Ld = np.longdouble
    dx = np.zeros((B, n)); dv = np.zeros((B, m)); ok = np.zeros(B, bool)
    for i in range(B):
        J, _ = QK.kkt_matrix(A[i], Pm[i], v[i], cones)
        if not np.isfinite(J).all() or np.linalg.cond(J) > 1e11:
            continue
        yh = QK._proj(v[i], cones)[0]
        Al, Pl, yl, vl, xl = (np.asarray(t, dtype=Ld) for t in (A[i], Pm[i], yh, v[i], x[i]))
        rhs = -np.concatenate([Pl @ xl + Al.T @ yl + c[i].astype(Ld), Al @ xl + (yl - vl) - b[i].astype(Ld)])
        d = np.linalg.solve(J, rhs.astype(np.float64)).astype(Ld)
        d = (d + np.linalg.solve(J, (rhs - J.astype(Ld) @ d).astype(np.float64)).astype(Ld)).astype(np.float64)
        ok[i] = True; dx[i], dv[i] = d[:n], d[n:]
    return dx, dv, ok


def distance(pt, x, v):
    """per instance: max(|x - x*|, |v - v*|) in the maximum norm, to the planted point"""
    return np.maximum(np.abs(x - pt["x"]).max(axis=1), np.abs(v - pt["v"]).max(axis=1))


def point(name, shape, **kw):
    """plant(shape) once per name: shared by the tests, not changed"""
    if name not in _POINTS:
        _POINTS[name] = plant(shape, **kw)
    return _POINTS[name]


# ---------------------------------------------------------------------------------------------- the shapes of tests/test_gpu_ns_mode_edges.py
def _all(shape_of_kind):
    return {k: shape_of_kind(k) for k in pk.NS_KIND_FIELD}


def _tri(kind, **kw):
    return kw if kind == "tri" else {}


# name -> {kind: shape}: the smallest shapes at which each thing exists (a kind that is not listed has no such shape)
STRUCTURE = {
    "n1": _all(lambda k: (k, 1, {"z": 0, "l": 3, "q": [], **_tri(k, ep=1, p=[])}, ())),                                  # npad = 2
    "n2_one_q3": _all(lambda k: (k, 2, {"z": 0, "l": 3, "q": [3], **_tri(k, ep=1, p=[])}, ("bd",))),
    "n3": _all(lambda k: (k, 3, {"z": 1, "l": 4, "q": [3], **_tri(k, ep=0, p=[0.3])}, ("bd",))),
    "z_is_n6": _all(lambda k: (k, 6, {"z": 6, "l": 3, "q": [3], **_tri(k, ep=1, p=[])}, ("out",))),                      # nf = 0: nothing to sweep
    "no_active_row": {"qp": ("qp", 8, {"z": 0, "l": 12, "q": [4]}, ("out",))},                                           # singular with a linear objective
    "q1_q2_blocks": _all(lambda k: (k, 6, {"z": 1, "l": 6, "q": [1, 2, 1, 2], **_tri(k, ep=1, p=[])}, ("in", "bd", "out", "in"))),
    "union_a_n28_twelve_q3": {k: (k, 28, {"z": 0, "l": 20, "q": [3] * 12}, ("bd",) * 12) for k in ("plain", "qp")},       # many cones: a_z and the publication buffers
    "union_c_n4_m400": {k: (k, 4, {"z": 1, "l": 396, "q": [3], **_tri(k, ep=1, p=[])}, ("bd",)) for k in ("plain", "tri")},                     # m + npad; more rows than threads, the cone's rows past row 256
    "union_b_n6": {k: (k, 6, {"z": 1, "l": 8, "q": [4]}, ("bd",)) for k in ("plain", "qp")},                              # the sweep buffers
}
STRUCTURE_ARGS = {"no_active_row": dict(active=0)}
UNION_LARGEST = {"union_a_n28_twelve_q3": 0, "union_c_n4_m400": 2, "union_b_n6": 1}


def edge_table():
    """[(family, kind, v_before, plan_before, v_after, plan_after)] of every NS family, from the host plan"""
    if "edges" not in _POINTS:
        _POINTS["edges"] = [(fam, pk.NS_FAMILIES[fam][0]) + e for fam in pk.NS_FAMILIES for e in pk.ns_edges(fam)]
    return _POINTS["edges"]


def edge_cases():
    """{name: (shape, host plan or None, what)}: both sides of every edge, each shape once.  what: "served", "refused" (the kind has no row), or "resolve" (a row,
    but the LSQR vectors of the re-solve do not fit: ce_jvp refused, ce_refine served)"""
    out = {}
    for fam, kind, vb, pb, va, pa in edge_table():
        for v, p in ((vb, pb), (va, pa)):
            what = "refused" if p is None else ("served" if p["resolve_fits"] or kind == "qp" else "resolve")
            out.setdefault(f"{fam}[{v}]", (pk.NS_FAMILIES[fam][2](v), p, what))
    return out


def structure_cases():
    """{name: (shape, host plan, "served")}"""
    return {f"{name}:{kind}": (shape, pk.host_ns_plan(shape), "served") for name, by in STRUCTURE.items() for kind, shape in by.items()}


def all_cases():
    return {**edge_cases(), **structure_cases()}


def cases_of(group):
    """the cases of a family of plan_kit.NS_FAMILIES (its edge shapes) or of one "structure shape:kind"""
    every = all_cases()
    return {k: c for k, c in every.items() if k == group or k.startswith(group + "[")}


def plant_args(name):
    return STRUCTURE_ARGS.get(name.split(":")[0], {})

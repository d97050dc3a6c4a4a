"""Shared by test_gpu_vjp_psd_many.py, test_gpu_jvp_psd_many.py and test_gpu_psd_many_edges.py: the points, right-hand sides and dense numpy references of the
many-cotangent adjoint and the many-tangent forward derivative with PSD blocks (k_backward_ns<..., MANY, PSD> behind ce_vjp_psd_many / ce_jvp_psd_many).  Nothing
here needs a GPU until a point is asked for; every reference is computed once per shape, shared, and not changed.

Shapes: the five of psd_ns_kit.SHAPES (rows 0 and 2 of CE_NS_VARIANTS) and the four edge shapes below (B = 8; n = 28 / 29 and 60 / 61 straddle the column limits
4 ceil(n / 4) + 1 <= 32 and <= 64 of rows 0 and 1).  Checked on the CPU with the oracle for these exact shapes and seeds: every instance is Solved, the dense systems
have condition numbers <= 1.4e3 (the edges) and <= 3e4 (the kit's), and the smallest min(B, 1 - B) of a weighted PSD row is 3.0e-3 (the edges), 3.4e-4 (the kit's):
nothing is filtered out of a reference and the stiff rule (1 - B < 1e-5) flags nothing, so the 0.8 share the tests ask for is the siblings' cap, not a measurement.

References, per instance, in solver form (A x + s = b), v = y - s, D = DPi(v) from psd_ns_kit.proj, J = psd_ns_kit.kkt_matrix(A, D) = [[0, A^T D], [A, D - I]]:
  forward  psd_ns_kit.dense_jvp:  J (d_x, d_v) = -(g_x, g_y);
  adjoint  J^T (r_x, r_y) = (dx, D dy),  dA = -(y r_x^T + r_y x^T),  db = r_y,  dc = -r_x  -- diffcp's adjoint with r_tau pinned to 0.  On these shapes and seeds it
           agrees with the oracle's adjoint_batch(mode="dense") to 1.7e-8 worst, <= 5.7e-10 median, relative to 1 + max |reference|."""
import numpy as np

import psd_ns_kit as K
from cvxpylayers_amd import problems as P

K_BEYOND = 17
KS = (1, 3, K_BEYOND)
ZERO_AT = 1          # position of the all-zero right-hand side (K >= 3); draw 0 is repeated at K - 1 (test_gpu_vjp_many.py's pattern)
MIN_SHARE = 0.8

# name -> (n, cones, B, seed, row of CE_NS_VARIANTS)
EDGES = {
    "edge_n28": (28, {"z": 3, "l": 12, "q": [6], "s": [4, 3]}, 8, 2, 0),
    "edge_n29": (29, {"z": 3, "l": 12, "q": [6], "s": [4, 3]}, 8, 2, 1),
    "edge_n60": (60, {"z": 4, "l": 30, "q": [8, 8], "s": [5, 4]}, 8, 4, 1),
    "edge_n61": (61, {"z": 4, "l": 30, "q": [8, 8], "s": [5, 4]}, 8, 4, 2),
}
_POINTS: dict = {}
_EDGE_PROBLEMS: dict = {}


def shape_of(name):
    return K.SHAPES[name] if name in K.SHAPES else EDGES[name][:4]


def problem(name):
    """(n, cones, A, b, c, the oracle's solution at eps 1e-10): psd_ns_kit's for its shapes, computed here for the edges"""
    if name in K.SHAPES:
        return K.problem(name)
    if name not in _EDGE_PROBLEMS:
        from oracle import oracle
        n, cones, B, seed = EDGES[name][:4]
        A, b, c = P.generate(n, cones, B, seed=seed)
        _EDGE_PROBLEMS[name] = (n, cones, A, b, c, oracle.solve_batch(A, b, c, cones, eps=1e-10, max_iters=200000))
    return _EDGE_PROBLEMS[name]


def draw_of(Kc, k):
    """the Gaussian draw at position k of a Kc-right-hand-side call (None: the zero one)"""
    if Kc >= 3 and k == ZERO_AT:
        return None
    return 0 if (Kc >= 3 and k == Kc - 1) else k


def pattern(Kc, *bases):
    """the first Kc draws of every base with zeros at ZERO_AT and draw 0 again at Kc - 1 when Kc >= 3"""
    out = []
    for base in bases:
        a = base[:Kc].copy()
        if Kc >= 3:
            a[ZERO_AT] = 0.0; a[Kc - 1] = base[0]
        out.append(a)
    return out


def dense_adjoint(A, x, y, s, dx, dy, cones, D=None):
    """{"dA" (B, m, n), "db" (B, m), "dc" (B, n)} of one cotangent (dx, dy) by the dense transposed system of the module docstring, and the condition numbers"""
    B, m, n = A.shape
    g = dict(dA=np.zeros((B, m, n)), db=np.zeros((B, m)), dc=np.zeros((B, n)))
    cond = np.zeros(B)
    for i in range(B):
        Di = D[i] if D is not None else K.proj(y[i] - s[i], cones)[1]
        J = K.kkt_matrix(A[i], Di)
        cond[i] = np.linalg.cond(J)
        r = np.linalg.solve(J.T, np.concatenate([dx[i], Di @ dy[i]]))
        rx, ry = r[:n], r[n:]
        g["dA"][i] = -(np.outer(y[i], rx) + np.outer(ry, x[i])); g["db"][i] = ry; g["dc"][i] = -rx
    return g, cond


def point(name, n_draws=K_BEYOND - 1):
    """problem, oracle point, engine, device tensors and the Gaussian draws of both directions; the dense references are added by want_adjoint / want_forward"""
    if name in _POINTS:
        return _POINTS[name]
    import torch
    from test_gpu_jvp import _engine, _tangents
    n, cones, A, b, c, ref = problem(name)
    assert (ref["status"] == 1).all(), ref["status"]
    tpl = P.dense_template(n, cones)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    B, seed = A.shape[0], shape_of(name)[3]
    rng = np.random.default_rng(seed + 1)
    base_dx = rng.standard_normal((K_BEYOND,) + ref["x"].shape); base_dy = rng.standard_normal((K_BEYOND,) + ref["y"].shape)
    base_tA = np.zeros((K_BEYOND, B, tpl.nnz_aug)); base_tq = np.zeros((K_BEYOND, B, n + 1)); dense_t = []
    for k in range(n_draws):
        d, tA_bm, tq = _tangents(tpl, B, seed=seed + 100 + k)
        base_tA[k] = tA_bm.cpu().numpy(); base_tq[k] = tq.cpu().numpy().T; dense_t.append(d)
    D = [K.proj(ref["y"][i] - ref["s"][i], cones)[1] for i in range(B)]
    margin = min(K.block_states(ref["y"][i] - ref["s"][i], cones)[1] for i in range(B))
    assert margin > 1e-5, (name, margin)          # the stiff rule flags nothing at these points
    r = dict(name=name, n=n, cones=cones, tpl=tpl, A=A, b=b, c=c, ref=ref, eng=_engine(tpl), A_bm=torch.from_numpy(A_eval).cuda().t().contiguous(),
             q_t=torch.from_numpy(q_eval).cuda(), pt=tuple(torch.from_numpy(ref[k]).cuda() for k in "xys"), base_dx=base_dx, base_dy=base_dy, base_tA=base_tA,
             base_tq=base_tq, dense_t=dense_t, D=D, n_draws=n_draws, want_adj={}, want_fwd={}, runs={})
    _POINTS[name] = r
    return r


def want_adjoint(r, d):
    """(dA in the engine's layout (B, nnz_aug), dc (B, n)) of Gaussian draw d"""
    if d not in r["want_adj"]:
        from test_gpu_ns_adjoint import _boundary
        ref = r["ref"]
        g, cond = dense_adjoint(r["A"], ref["x"], ref["y"], ref["s"], r["base_dx"][d], r["base_dy"][d], r["cones"], D=r["D"])
        assert (cond <= 1e11).all() and np.isfinite(g["dA"]).all(), (r["name"], cond.max())          # nothing left out
        r["want_adj"][d] = (_boundary(r["tpl"], g, r["n"]).T, g["dc"])
    return r["want_adj"][d]


def want_forward(r, d):
    """(dx, dy, ds) of Gaussian tangent draw d (psd_ns_kit.dense_jvp)"""
    if d not in r["want_fwd"]:
        ref = r["ref"]
        w = K.dense_jvp(r["A"], ref["x"], ref["y"], ref["s"], *r["dense_t"][d], r["cones"])
        assert w[3].all(), (r["name"], d, w[4])          # nothing left out
        r["want_fwd"][d] = w[:3]
    return r["want_fwd"][d]


def rel(got, want):
    return np.abs(got - want).max(axis=-1) / (1 + np.abs(want).max(axis=-1))


def run_vjp(r, Kc, loop=False):
    """vjp_many(psd_many=True) -- or the loop of pivoting ce_vjp calls (force_loop=True) -- for Kc cotangents at the shape's point (once each): device tensors"""
    import torch
    from kit import TIGHT_LSQR
    key = ("vjp", Kc, loop)
    if key not in r["runs"]:
        eng = r["eng"]
        dx, dy = (torch.from_numpy(a).cuda() for a in pattern(Kc, r["base_dx"], r["base_dy"]))
        got = eng.vjp_many(r["A_bm"], *r["pt"], dx, dy, path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], psd_many=True, force_loop=loop)
        r["runs"][key] = dict(path=eng.last_vjp_many_path, kernel=eng.last_vjp_kernel, out=tuple(got), dx=dx, dy=dy)
        torch.cuda.synchronize()
    return r["runs"][key]


def run_jvp(r, Kc, loop=False):
    """jvp_many(psd_many=True) -- or the loop of ce_jvp_psd calls (force_loop=True) -- for Kc tangents: device tensors (dx, dy, ds, status, iters)"""
    import torch
    from kit import TIGHT_LSQR
    key = ("jvp", Kc, loop)
    if key not in r["runs"]:
        eng = r["eng"]
        tA, tq = (torch.from_numpy(a).cuda() for a in pattern(Kc, r["base_tA"], r["base_tq"]))
        got = eng.jvp_many(r["A_bm"], *r["pt"], tA, tq, q_eval=r["q_t"], psd_many=True, force_loop=loop, path="per_instance", lsqr=TIGHT_LSQR, method="direct")
        r["runs"][key] = dict(path=eng.last_jvp_many_path, kernel=eng.last_jvp_kernel, out=tuple(got) + (eng.last_lsqr_iters,), tA=tA, tq=tq)
        torch.cuda.synchronize()
    return r["runs"][key]


def check_vjp_against_dense(r, Kc):
    """every cotangent of a Kc call against the dense reference, on status-0 instances (>= MIN_SHARE): 1e-5 worst, 1e-8 median relative to 1 + max |reference|"""
    o = run_vjp(r, Kc)
    assert o["path"] == "many" and o["kernel"] == "ce_vjp_psd_many", (o["path"], o["kernel"])
    dA, dq, adj = (t.cpu().numpy() for t in o["out"])
    n, B = r["n"], r["A"].shape[0]
    assert dA.shape == (Kc, B, r["tpl"].nnz_aug) and dq.shape == (Kc, B, n + 1) and adj.shape == (Kc, B)
    assert (dq[:, :, n] == 0).all()
    for k in range(Kc):
        d = draw_of(Kc, k)
        reg = adj[k] == 0
        assert reg.mean() >= MIN_SHARE, (r["name"], Kc, k, reg.mean(), np.bincount(adj[k]))
        if d is None:
            continue
        wA, wc = want_adjoint(r, d)
        e, ec = rel(dA[k], wA)[reg], rel(dq[k][:, :n], wc)[reg]
        print(f"{r['name']} K={Kc} k={k}: dA worst {e.max():.2e} median {np.median(e):.2e}, dc worst {ec.max():.2e} median {np.median(ec):.2e}, compared {reg.mean():.3f}, "
              f"status counts {np.bincount(adj[k]).tolist()}")
        assert e.max() < 1e-5 and np.median(e) < 1e-8, (r["name"], Kc, k, e.max(), np.median(e))
        assert ec.max() < 1e-5 and np.median(ec) < 1e-8, (r["name"], Kc, k, ec.max(), np.median(ec))


def check_jvp_against_dense(r, Kc):
    """every tangent of a Kc call against psd_ns_kit.dense_jvp, on status-0 instances (>= MIN_SHARE, no iteration there): the same two bounds"""
    o = run_jvp(r, Kc)
    assert o["path"] == "many" and o["kernel"] == "ce_jvp_psd_many", (o["path"], o["kernel"])
    dx, dy, ds, st, its = (t.cpu().numpy() for t in o["out"])
    n, m, B = r["n"], r["tpl"].m, r["A"].shape[0]
    assert dx.shape == (Kc, B, n) and dy.shape == ds.shape == (Kc, B, m) and st.shape == its.shape == (Kc, B)
    for k in range(Kc):
        d = draw_of(Kc, k)
        reg = st[k] == 0
        assert reg.mean() >= MIN_SHARE, (r["name"], Kc, k, reg.mean(), np.bincount(st[k]))
        assert (its[k][reg] == 0).all(), (r["name"], Kc, k)
        if d is None:
            continue
        for got, want, what in zip((dx[k], dy[k], ds[k]), want_forward(r, d), ("dx", "dy", "ds")):
            e = rel(got, want)[reg]
            print(f"{r['name']} K={Kc} k={k}: {what} worst {e.max():.2e} median {np.median(e):.2e}, compared {reg.mean():.3f}, status counts {np.bincount(st[k]).tolist()}")
            assert e.max() < 1e-5 and np.median(e) < 1e-8, (r["name"], Kc, k, what, e.max(), np.median(e))

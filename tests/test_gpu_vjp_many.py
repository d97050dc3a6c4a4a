"""K cotangents at one solution on one factorisation per instance: k_backward_ns<..., MANY> behind ce_vjp_many, ConeEngine.vjp_many.

Shapes and seeds are test_gpu_ns_adjoint.py's (the oracle converges on them and the regular share holds); the tile-variant edges n = 28 / 29 / 59 / 60 replay the
generator of its sweep, so the patterns and values are the ones it draws.  Every result is checked twice: against the oracle's dense elimination of the full M^T
(1e-5 worst, 1e-8 median, the existing test's bounds) and against the same engine's loop of K vjp calls (1e-6 on every instance, flagged ones included; equal flags).

The kernel takes the cotangents one after the other on the retained factors: it has no chunk and no packed pass, so no per-pass capacity.  K_BEYOND = 17 is the value
the specification sets for that case.  Cotangents are independent Gaussians; cotangent 0 is repeated at position K - 1 (state left over from one right-hand side to
the next shows as a difference between the two) and one cotangent is all zeros (exact zeros come back on unflagged instances)."""
import numpy as np
import pytest
import torch

from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR
from test_gpu_ns_adjoint import _boundary
from test_gpu_parity import _engine_for, gpu_solve

pytestmark = pytest.mark.gpu

K_BEYOND = 17
KS = (1, 3, K_BEYOND)
ZERO_AT = 1          # position of the all-zero cotangent (K >= 3)

# name -> (n, cones, B, seed, eps, least regular share)
FIXED = {
    "small_mixed": (12, {"z": 2, "l": 6, "q": [4, 5]}, 48, 1, 1e-9, 0.8),
    "ragged_cones": (20, {"z": 3, "l": 10, "q": [3, 7, 2, 5, 1]}, 48, 4, 1e-9, 0.8),
    "soc_only": (25, {"z": 0, "l": 0, "q": [6] * 6}, 32, 5, 1e-9, 0.8),
    "M": (P.CONFIGS["M"]["n"], P.CONFIGS["M"]["cones"], 64, 3, 1e-9, 0.95),
    "C3": (P.CONFIGS["C3"]["n"], P.CONFIGS["C3"]["cones"], 8, 7, 1e-9, 0.9),
}
EDGES = ("edge_n28", "edge_n29", "edge_n59", "edge_n60")
SHAPES = tuple(FIXED) + EDGES
_CACHE: dict = {}
_SWEEP: dict = {}


# what the oracle does with the shapes of that sweep at eps 1e-9 (it converges on fewer than four of 24 instances of these, and the sweep passes them over): not solved
# again here -- 200000 iterations each -- but the sweep's draws for them are made, so that the later shapes get the patterns and seeds they get there
SWEEP_UNSOLVED = (16, 28, 59)
# the planted points of the two edges among them (ns_edge_kit: the adjoint is a linear system AT a point): cone states and active nonnegative rows that leave the
# system regular with a reduced Hessian to sweep -- n = 28: k1 = 21 unit directions, L = 7 weighted ones, nf = 7; n = 59: k1 = 37, L = 25, nf = 22
PLANTED = {28: (("in", "bd", "in"), 10), 59: (("bd", "bd", "bd"), 30)}


def _sweep():
    """the shapes of test_random_templates_sparse_patterns_and_edge_shapes_against_the_pivoting_kernel, drawn from its generator in its order (the draws it makes
    for its own cotangents are made and dropped): name -> (n, cones, pattern, A, b, c, point).  Solved instances only, as there; a planted point on the sweep's
    pattern where the oracle does not converge."""
    if _SWEEP:
        return _SWEEP
    from oracle import oracle
    import ns_edge_kit as E
    rng = np.random.default_rng(2024)
    shapes = [(1, {"z": 0, "l": 3, "q": []}, 1.0), (5, {"z": 1, "l": 4, "q": [3]}, 0.6), (9, {"z": 0, "l": 0, "q": [4, 3, 5]}, 0.7), (16, {"z": 3, "l": 12, "q": []}, 0.5),
              (28, {"z": 2, "l": 10, "q": [6, 9, 2]}, 0.4), (29, {"z": 0, "l": 16, "q": [8, 8]}, 1.0), (59, {"z": 4, "l": 30, "q": [12, 12, 7]}, 0.3), (60, {"z": 0, "l": 40, "q": [10] * 4}, 1.0)]
    for n, cones, dens in shapes:
        m = P.cone_rows(cones)
        pat = rng.random((m, n)) < dens
        pat[np.arange(m), rng.integers(0, n, m)] = True
        pat[rng.integers(0, m, n), np.arange(n)] = True
        seed = int(rng.integers(1 << 30))
        if n in SWEEP_UNSOLVED:
            if n in PLANTED:
                pt = E.plant(("lin", n, cones, PLANTED[n][0]), B=24, seed=seed, active=PLANTED[n][1])
                A = pt["A"] * pat[None]          # (the point stays a KKT point of the masked matrix with its own b and c)
                b = np.einsum("bij,bj->bi", A, pt["x"]) + pt["s"]; c = -np.einsum("bij,bi->bj", A, pt["y"])
                _SWEEP[f"edge_n{n}"] = (n, cones, pat, A, b, c, dict(x=pt["x"], y=pt["y"], s=pt["s"], status=np.ones(24, int), planted=True))
            continue
        A, b, c = P.generate(n, cones, 24, seed=seed)
        A = A * pat[None]
        ref = oracle.solve_batch(A, b, c, cones, eps=1e-9, max_iters=200000)
        ok = ref["status"] == 1
        assert ok.sum() >= 4, (n, ok.sum())
        A, b, c = A[ok], b[ok], c[ok]; ref = {k: v[ok] for k, v in ref.items()}
        rng.standard_normal(ref["x"].shape); rng.standard_normal(ref["y"].shape)          # (plain-cone templates with n <= 108 all have the search-free adjoint: the sweep draws here)
        _SWEEP[f"edge_n{n}"] = (n, cones, pat, A, b, c, ref)
    return _SWEEP


def cotangents(K, base_dx, base_dy):
    """(K, B, n), (K, B, m) from K_BEYOND - 1 Gaussian draws: draw k at position k, the zero cotangent at ZERO_AT and draw 0 again at K - 1 when K >= 3"""
    dx, dy = base_dx[:K].copy(), base_dy[:K].copy()
    if K >= 3:
        dx[ZERO_AT] = 0.0; dy[ZERO_AT] = 0.0
        dx[K - 1] = base_dx[0]; dy[K - 1] = base_dy[0]
    return dx, dy


def _point(name):
    """problem, oracle point, engine, Gaussian draws and the oracle's dense adjoint of every draw: computed once per shape, shared, not changed"""
    if name in _CACHE:
        return _CACHE[name]
    from oracle import oracle
    if name in FIXED:
        n, cones, B, seed, eps, share = FIXED[name]
        tpl = P.dense_template(n, cones)
        A, b, c = P.generate(n, cones, B, seed=seed)
        ref = oracle.solve_batch(A, b, c, cones, eps=eps, max_iters=200000)
    else:
        n, cones, pat, A, b, c, ref = _sweep()[name]
        tpl = P.dense_template(n, cones, pattern=pat)
        seed, eps, share = n, 1e-9, 0.8
    ok = ref["status"] == 1
    if ref.get("planted"):          # (nothing to solve for: the engine and the batch-major values alone)
        eng = _engine_for(tpl)
        A_bm = eng.to_batch_major(torch.from_numpy(tpl.values_from_dense(A, b, c)[0]).cuda())
    else:
        eng, A_bm, *_ = gpu_solve(tpl, A, b, c, eps=eps, max_iters=200000)
    rng = np.random.default_rng(seed + 1)
    base_dx = rng.standard_normal((K_BEYOND,) + ref["x"].shape); base_dy = rng.standard_normal((K_BEYOND,) + ref["y"].shape)
    gs = [oracle.adjoint_batch(A, b, c, cones, ref["x"], ref["y"], ref["s"], base_dx[k], base_dy[k], mode="dense") for k in range(K_BEYOND - 1)]
    want, dc = [_boundary(tpl, g, n).T for g in gs], [g["dc"] for g in gs]
    _, q_eval = tpl.values_from_dense(A, b, c)
    r = dict(name=name, n=n, cones=cones, tpl=tpl, A=A, b=b, c=c, ref=ref, ok=ok, eng=eng, A_bm=A_bm, q_t=torch.from_numpy(q_eval).cuda(), share=share,
             pt=tuple(torch.from_numpy(ref[k]).cuda() for k in "xys"), base_dx=base_dx, base_dy=base_dy, want=want, dc=dc, runs={})
    _CACHE[name] = r
    return r


def _run(r, K):
    """vjp_many and its loop for K cotangents at the shape's point (once per K)"""
    if K in r["runs"]:
        return r["runs"][K]
    eng = r["eng"]
    dx, dy = cotangents(K, r["base_dx"], r["base_dy"])
    dxt, dyt = torch.from_numpy(dx).cuda(), torch.from_numpy(dy).cuda()
    many = eng.vjp_many(r["A_bm"], *r["pt"], dxt, dyt, path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"])
    path = eng.last_vjp_many_path
    loop = eng.vjp_many(r["A_bm"], *r["pt"], dxt, dyt, path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], force_loop=True)
    assert eng.last_vjp_many_path == "loop"
    torch.cuda.synchronize()
    out = dict(path=path, many=tuple(t.cpu().numpy() for t in many), loop=tuple(t.cpu().numpy() for t in loop))
    r["runs"][K] = out
    return out


def _draw_of(K, k):
    """the Gaussian draw at position k of a K-cotangent call (None: the zero cotangent)"""
    if K >= 3 and k == ZERO_AT:
        return None
    return 0 if (K >= 3 and k == K - 1) else k


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", SHAPES)
def test_every_cotangent_against_the_oracles_dense_adjoint(name, K):
    r = _point(name)
    o = _run(r, K)
    assert o["path"] == "many"
    dA, dq, adj = o["many"]
    n = r["n"]
    assert dA.shape == (K, len(r["ok"]), r["tpl"].nnz_aug) and dq.shape == (K, len(r["ok"]), n + 1) and adj.shape == (K, len(r["ok"]))
    assert (dq[:, :, n] == 0).all()
    for k in range(K):
        d = _draw_of(K, k)
        if d is None:
            continue
        want = r["want"][d]
        reg = r["ok"] & (adj[k] == 0)
        assert reg.mean() >= r["share"], (name, K, k, reg.mean(), np.bincount(adj[k]))
        e = (np.abs(dA[k] - want).max(axis=1) / (1 + np.abs(want).max(axis=1)))[reg]
        print(f"{name} K={K} k={k}: dA worst {e.max():.2e} median {np.median(e):.2e}, regular {reg.mean():.3f}")
        assert e.max() < 1e-5 and np.median(e) < 1e-8, (name, K, k, e.max(), np.median(e))
        edc = (np.abs(dq[k][:, :n] - r["dc"][d]).max(axis=1) / (1 + np.abs(r["dc"][d]).max(axis=1)))[reg]
        print(f"{name} K={K} k={k}: dc worst {edc.max():.2e} median {np.median(edc):.2e}")
        assert edc.max() < 1e-5 and np.median(edc) < 1e-8, (name, K, k, edc.max(), np.median(edc))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", SHAPES)
def test_every_cotangent_against_the_loop_of_single_cotangent_calls(name, K):
    r = _point(name)
    o = _run(r, K)
    assert o["path"] == "many"
    (dA, dq, adj), (dA_l, dq_l, adj_l) = o["many"], o["loop"]
    assert (adj == adj_l).all(), (name, K, adj, adj_l)
    assert ((adj & (4 | 8)) == (adj[:1] & (4 | 8))).all()          # rank deficiency is the matrix's: the same for every cotangent
    eA = np.abs(dA - dA_l).max(axis=2) / (1 + np.abs(dA_l).max(axis=2))
    eq = np.abs(dq - dq_l).max(axis=2) / (1 + np.abs(dq_l).max(axis=2))
    print(f"{name} K={K}: against the loop dA {eA.max():.2e} dq {eq.max():.2e}, flagged {int((adj[0] != 0).sum())}")
    assert eA.max() < 1e-6 and eq.max() < 1e-6, (name, K, eA.max(), eq.max())
    if K >= 3:
        un = adj[ZERO_AT] == 0
        assert (dA[ZERO_AT][un] == 0).all() and (dq[ZERO_AT][un] == 0).all()
        e0 = np.abs(dA[0] - dA[K - 1]).max(axis=1) / (1 + np.abs(dA[0]).max(axis=1))          # the repeated cotangent, first and last
        print(f"{name} K={K}: cotangent 0 against its repeat {e0.max():.2e}")
        assert e0.max() < 1e-6, (name, K, e0.max())


def test_duplicated_equality_rows_are_flagged_for_every_cotangent_and_resolved():
    from oracle import oracle
    n, cones, B, K = 12, {"z": 4, "l": 8, "q": [5]}, 24, 3
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=11)
    deg = np.arange(B) % 2 == 0
    A[deg, 2, :] = A[deg, 0, :]; b[deg, 2] = b[deg, 0]
    ref = oracle.solve_batch(A, b, c, cones, eps=1e-10, max_iters=200000)
    keep = ref["status"] == 1
    assert keep.mean() > 0.8
    A, b, c, deg = A[keep], b[keep], c[keep], deg[keep]
    ref = {k: v[keep] for k, v in ref.items()}
    eng, A_bm, *_ = gpu_solve(tpl, A, b, c, eps=1e-10, max_iters=200000)
    rng = np.random.default_rng(12)
    dx = rng.standard_normal((K,) + ref["x"].shape); dy = rng.standard_normal((K,) + ref["y"].shape)
    _, q_eval = tpl.values_from_dense(A, b, c)
    dA, dq, adj = eng.vjp_many(A_bm, *(torch.from_numpy(ref[k]).cuda() for k in "xys"), torch.from_numpy(dx).cuda(), torch.from_numpy(dy).cuda(), path="per_instance",
                               lsqr=TIGHT_LSQR, q_eval=torch.from_numpy(q_eval).cuda())
    assert eng.last_vjp_many_path == "many"
    torch.cuda.synchronize()
    a, dA = adj.cpu().numpy(), dA.cpu().numpy()
    for k in range(K):
        assert (a[k][deg] == 12).all() and (a[k][~deg] == 0).all(), (k, a[k])
        g = oracle.adjoint_batch(A, b, c, cones, ref["x"], ref["y"], ref["s"], dx[k], dy[k], mode="lsqr", lsqr_atol=TIGHT_LSQR[0], lsqr_btol=TIGHT_LSQR[1], lsqr_iter_lim=TIGHT_LSQR[2])
        want = _boundary(tpl, g, n).T
        err = np.abs(dA[k] - want).max()
        print(f"duplicated rows k={k}: {err:.2e} against {1e-6 * (1 + np.abs(want).max()):.2e}")
        assert err < 1e-6 * (1 + np.abs(want).max()), (k, err)


def test_lp_vertices_are_flagged_or_solved_for_every_cotangent():
    from oracle import oracle
    n, cones, B, K = 10, {"z": 0, "l": 30, "q": []}, 64, 3
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=9)
    ref = oracle.solve_batch(A, b, c, cones, eps=1e-10, max_iters=200000)
    ok = ref["status"] == 1
    assert ok.mean() > 0.9
    eng, A_bm, *_ = gpu_solve(tpl, A, b, c, eps=1e-10, max_iters=200000)
    rng = np.random.default_rng(10)
    dx = rng.standard_normal((K,) + ref["x"].shape); dy = rng.standard_normal((K,) + ref["y"].shape)
    _, q_eval = tpl.values_from_dense(A, b, c)
    dA, dq, adj = eng.vjp_many(A_bm, *(torch.from_numpy(ref[k]).cuda() for k in "xys"), torch.from_numpy(dx).cuda(), torch.from_numpy(dy).cuda(), path="per_instance",
                               lsqr=TIGHT_LSQR, q_eval=torch.from_numpy(q_eval).cuda())
    assert eng.last_vjp_many_path == "many"
    torch.cuda.synchronize()
    a, dA = adj.cpu().numpy(), dA.cpu().numpy()
    for k in range(K):
        reg = ok & (a[k] == 0)
        assert reg.mean() > 0.5
        want = _boundary(tpl, oracle.adjoint_batch(A, b, c, cones, ref["x"], ref["y"], ref["s"], dx[k], dy[k], mode="dense"), n).T
        e = (np.abs(dA[k] - want).max(axis=1) / (1 + np.abs(want).max(axis=1)))[reg]
        print(f"LP vertices k={k}: unflagged worst {e.max():.2e} median {np.median(e):.2e}, regular {reg.mean():.3f}")
        assert e.max() < 1e-5 and np.median(e) < 1e-8, (k, e.max(), np.median(e))
        fl = (a[k] & 8) != 0
        assert ((a[k] & 4) != 0).sum() == fl.sum() and (fl == ((a[0] & 8) != 0)).all()
        if fl.any():
            assert ((a[k][fl] & 3) == 0).all()
            idx = np.nonzero(fl)[0]
            gl = oracle.adjoint_batch(A[idx], b[idx], c[idx], cones, ref["x"][idx], ref["y"][idx], ref["s"][idx], dx[k][idx], dy[k][idx], mode="lsqr",
                                      lsqr_atol=TIGHT_LSQR[0], lsqr_btol=TIGHT_LSQR[1], lsqr_iter_lim=TIGHT_LSQR[2])
            wl = _boundary(tpl, gl, n).T
            el = np.abs(dA[k][idx] - wl).max(axis=1) / (1 + np.abs(wl).max(axis=1))
            print(f"LP vertices k={k}: flagged {fl.sum()} worst {el.max():.2e} median {np.median(el):.2e}")
            assert np.median(el) < 1e-6 and el.max() < 5e-3, (k, el)


def _raw_many(eng, B, K, A_bm, q_t, x, y, s, dx):
    f64 = dict(dtype=torch.float64, device="cuda")
    dA = torch.empty((K, B, eng.nnz_aug), **f64); dq = torch.empty((K, B, eng.n + 1), **f64)
    rc = _lib.lib().ce_vjp_many(eng._h, B, K, A_bm.data_ptr(), eng.nnz_aug, q_t.data_ptr(), q_t.stride(0), q_t.stride(1), x.data_ptr(), y.data_ptr(), s.data_ptr(),
                                dx.data_ptr(), None, dA.data_ptr(), dq.data_ptr(), None, None)
    return rc, (_lib.lib().ce_last_error() or b"").decode()


def test_a_template_with_an_exponential_triple_runs_the_loop():
    from oracle import oracle
    n, cones, B, K = 6, {"z": 1, "l": 3, "q": [4], "ep": 1}, 8, 3
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=1)
    ref = oracle.solve_batch(A, b, c, cones, eps=1e-9, max_iters=200000)
    eng, A_bm, *_ = gpu_solve(tpl, A, b, c, eps=1e-9, max_iters=200000)
    assert _lib.lib().ce_vjp_many_variant(eng._h) < 0
    pt = tuple(torch.from_numpy(np.nan_to_num(ref[k])).cuda() for k in "xys")
    rng = np.random.default_rng(2)
    dx = torch.from_numpy(rng.standard_normal((K, B, n))).cuda(); dy = torch.from_numpy(rng.standard_normal((K, B, tpl.m))).cuda()
    _, q_eval = tpl.values_from_dense(A, b, c); q_t = torch.from_numpy(q_eval).cuda()
    dA, dq, adj = eng.vjp_many(A_bm, *pt, dx, dy, path="per_instance", lsqr=TIGHT_LSQR, q_eval=q_t)
    assert eng.last_vjp_many_path == "loop"
    for k in range(K):
        a1, q1, s1 = eng.vjp(A_bm, *pt, dx[k], dy[k], path="per_instance", lsqr=TIGHT_LSQR, q_eval=q_t)
        assert torch.equal(dA[k], a1.t()) and torch.equal(dq[k], q1.t()) and torch.equal(adj[k], s1)
    rc, msg = _raw_many(eng, B, K, A_bm.contiguous(), q_t, *pt, dx)
    assert rc == -2 and "ce_vjp_many" in msg and "exponential" in msg, (rc, msg)


def test_a_template_with_a_native_quadratic_objective_runs_the_loop_and_returns_dP():
    import qp_ns_kit as Q
    from test_quad_objective import _upper_structure
    from cvxpylayers_amd.interfaces.mi355_if import make_settings
    n, cones, A, b, c, Pm = Q.instance("small_mixed")
    tpl = P.dense_template(n, cones)
    struct = _upper_structure(n)
    eng = Q.qp_engine(tpl, struct)
    assert eng.qp_native and _lib.lib().ce_vjp_many_variant(eng._h) < 0
    A_bm, q_t, P_bm = Q.device_values(tpl, A, b, c, Pm, struct)
    x, y, s, *_ = eng.solve(A_bm, q_t, make_settings(dict(eps=1e-9, max_iters=200000, acceleration_lookback=0)), P_bm=P_bm)
    B, K = A.shape[0], 3
    rng = np.random.default_rng(3)
    dx = torch.from_numpy(rng.standard_normal((K, B, n))).cuda(); dy = torch.from_numpy(rng.standard_normal((K, B, tpl.m))).cuda()
    dA, dq, adj, dP = eng.vjp_many(A_bm, x, y, s, dx, dy, path="per_instance", q_eval=q_t, P_bm=P_bm)
    assert eng.last_vjp_many_path == "loop" and dP.shape == (K, B, eng.nnz_p)
    for k in range(K):
        a1, q1, s1, p1 = eng.vjp(A_bm, x, y, s, dx[k], dy[k], path="per_instance", q_eval=q_t, P_bm=P_bm)
        assert torch.equal(dA[k], a1.t()) and torch.equal(dq[k], q1.t()) and torch.equal(adj[k], s1) and torch.equal(dP[k], p1)
    rc, msg = _raw_many(eng, B, K, A_bm.contiguous(), q_t, x, y, s, dx)
    assert rc == -2 and "quadratic objective" in msg, (rc, msg)


def test_empty_batches_and_no_cotangent_return_empty_tensors():
    r = _point("small_mixed")
    eng, B, n, m = r["eng"], len(r["ok"]), r["n"], r["tpl"].m
    z = torch.zeros((0, B, n), dtype=torch.float64, device="cuda")
    dA, dq, adj = eng.vjp_many(r["A_bm"], *r["pt"], z, None, path="per_instance", q_eval=r["q_t"])
    assert dA.shape == (0, B, eng.nnz_aug) and dq.shape == (0, B, n + 1) and adj.shape == (0, B)
    e = torch.zeros((0, m), dtype=torch.float64, device="cuda")
    dA, dq, adj = eng.vjp_many(r["A_bm"][:0], e[:, :n], e, e, torch.zeros((2, 0, n), dtype=torch.float64, device="cuda"), None, path="per_instance", q_eval=r["q_t"][:, :0])
    assert dA.shape == (2, 0, eng.nnz_aug) and dq.shape == (2, 0, n + 1) and adj.shape == (2, 0)


def test_a_null_dy_is_the_zero_cotangent():
    r = _point("small_mixed")
    eng = r["eng"]
    dx, dy = cotangents(3, r["base_dx"], r["base_dy"])
    dxt = torch.from_numpy(dx).cuda()
    a = eng.vjp_many(r["A_bm"], *r["pt"], dxt, None, path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"])
    assert eng.last_vjp_many_path == "many"
    b = eng.vjp_many(r["A_bm"], *r["pt"], dxt, torch.zeros_like(torch.from_numpy(dy)).cuda(), path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"])
    assert all(torch.equal(u, v) for u, v in zip(a, b))

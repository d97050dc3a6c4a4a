"""K cotangents at one solution of a template with exponential / power triples on one factorisation per instance: k_backward_ns<..., TRI, MANY> (no FWD) behind
ce_vjp_tri_many, ConeEngine.vjp_many(tri_many=True).

Shapes are tri_ns_kit.SHAPES, all five (exp_small n = 6 and triples_only -- no plain row at all -- are the smallest at which the triples' code can go wrong; E and
row2_n80 reach rows 1 and 2 of CE_NS_VARIANTS); the linearisation points are the oracle's (eps 1e-10, every instance Solved).  K and the cotangent pattern are
test_gpu_vjp_many's: K in (1, 3, 17), cotangent 0 repeated at K - 1, an all-zero cotangent at position 1.  Checked against
  * the oracle's dense elimination of the full M^T (adjoint_batch(mode="dense"), then _boundary): 1e-5 worst, 1e-8 median relative to 1 + max |reference| on every
    instance with status 0, which must be >= 80 % for every k;
  * the same engine's loop of K pivoting ce_vjp calls (force_loop=True): 1e-6 where both routes report status 0 (>= 80 %);
  * the transpose identity against ce_jvp (k_backward_ns<..., FWD, TRI>);
  * duplicated equality rows (flagged for every k, listed once, re-solved by LSQR per cotangent);
  * the defaults and refusals that stay."""
import numpy as np
import pytest
import torch

import tri_ns_kit as K
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR
from test_gpu_jvp import _engine, _tangents
from test_gpu_ns_adjoint import _boundary
from test_gpu_vjp_many import KS, K_BEYOND, ZERO_AT, _draw_of, cotangents

pytestmark = pytest.mark.gpu
_CACHE: dict = {}
MIN_SHARE = 0.8
SNAP = 1e-9


def _point(name):
    """problem, oracle point, engine, Gaussian draws and the oracle's dense adjoint of every draw: computed once per shape, shared, not changed"""
    if name in _CACHE:
        return _CACHE[name]
    from oracle import oracle
    n, cones, A, b, c, ref = K.problem(name)
    assert (ref["status"] == 1).all(), ref["status"]
    tpl = P.dense_template(n, cones)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    rng = np.random.default_rng(K.SHAPES[name][3] + 1)
    base_dx = rng.standard_normal((K_BEYOND,) + ref["x"].shape); base_dy = rng.standard_normal((K_BEYOND,) + ref["y"].shape)
    gs = [oracle.adjoint_batch(A, b, c, cones, ref["x"], ref["y"], ref["s"], base_dx[k], base_dy[k], mode="dense") for k in range(K_BEYOND - 1)]
    assert all(np.isfinite(g["dA"]).all() and np.isfinite(g["db"]).all() and np.isfinite(g["dc"]).all() for g in gs), name          # nothing left out on the oracle's side
    # the smallest 1 - lambda of a weighted triple row per instance (1 where it has none)
    stiff = np.ones(A.shape[0])
    for i in range(A.shape[0]):
        ev = K.triple_states(ref["y"][i] - ref["s"][i], cones)
        mid = ev[(ev > SNAP) & (ev < 1 - SNAP)]
        if mid.size:
            stiff[i] = (1 - mid).min()
    r = dict(name=name, n=n, cones=cones, tpl=tpl, A=A, b=b, c=c, ref=ref, eng=_engine(tpl), A_bm=torch.from_numpy(A_eval).cuda().t().contiguous(),
             q_t=torch.from_numpy(q_eval).cuda(), pt=tuple(torch.from_numpy(ref[k]).cuda() for k in "xys"), base_dx=base_dx, base_dy=base_dy,
             want=[_boundary(tpl, g, n).T for g in gs], dc=[g["dc"] for g in gs], stiff=stiff, runs={})
    _CACHE[name] = r
    return r


def _run(r, Kc, loop=False):
    """vjp_many(tri_many=True) -- and, asked for, the loop of pivoting calls -- for Kc cotangents at the shape's point (once each)"""
    key = (Kc, loop)
    if key in r["runs"]:
        return r["runs"][key]
    eng = r["eng"]
    dx, dy = cotangents(Kc, r["base_dx"], r["base_dy"])
    dxt, dyt = torch.from_numpy(dx).cuda(), torch.from_numpy(dy).cuda()
    got = eng.vjp_many(r["A_bm"], *r["pt"], dxt, dyt, path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], tri_many=not loop, force_loop=loop)
    path, kernel = eng.last_vjp_many_path, eng.last_vjp_kernel
    torch.cuda.synchronize()
    out = dict(path=path, kernel=kernel, out=tuple(t.cpu().numpy() for t in got))
    r["runs"][key] = out
    return out


@pytest.mark.parametrize("Kc", KS)
@pytest.mark.parametrize("name", list(K.SHAPES))
def test_every_cotangent_against_the_oracles_dense_adjoint(name, Kc):
    """fails on a tree without the mode: vjp_many takes no tri_many there"""
    r = _point(name)
    o = _run(r, Kc)
    assert o["path"] == "many" and o["kernel"] == "ce_vjp_tri_many", (o["path"], o["kernel"])
    assert _lib.lib().ce_vjp_tri_many_variant(r["eng"]._h) == K.SHAPES[name][4] == _lib.lib().ce_tri_ns_variant(r["eng"]._h)
    assert _lib.lib().ce_vjp_many_variant(r["eng"]._h) == -1 and _lib.lib().ce_adjoint_ns_variant(r["eng"]._h) == -1
    dA, dq, adj = o["out"]
    n, B = r["n"], r["A"].shape[0]
    assert dA.shape == (Kc, B, r["tpl"].nnz_aug) and dq.shape == (Kc, B, n + 1) and adj.shape == (Kc, B)
    assert (dq[:, :, n] == 0).all()
    for k in range(Kc):
        d = _draw_of(Kc, k)
        reg = adj[k] == 0
        assert reg.mean() >= MIN_SHARE, (name, Kc, k, reg.mean(), np.bincount(adj[k]))
        if d is None:
            continue
        want = r["want"][d]
        e = (np.abs(dA[k] - want).max(axis=1) / (1 + np.abs(want).max(axis=1)))[reg]
        edc = (np.abs(dq[k][:, :n] - r["dc"][d]).max(axis=1) / (1 + np.abs(r["dc"][d]).max(axis=1)))[reg]
        print(f"{name} K={Kc} k={k}: dA worst {e.max():.2e} median {np.median(e):.2e}, dc worst {edc.max():.2e} median {np.median(edc):.2e}, compared {reg.mean():.3f}, "
              f"status counts {np.bincount(adj[k]).tolist()}, smallest 1 - lambda of a weighted triple row among the compared {r['stiff'][reg].min():.2e}")
        assert e.max() < 1e-5 and np.median(e) < 1e-8, (name, Kc, k, e.max(), np.median(e))
        assert edc.max() < 1e-5 and np.median(edc) < 1e-8, (name, Kc, k, edc.max(), np.median(edc))


@pytest.mark.parametrize("Kc", KS)
@pytest.mark.parametrize("name", ["exp_pow_mixed", "E"])
def test_every_cotangent_against_the_loop_of_pivoting_calls(name, Kc):
    r = _point(name)
    o, l = _run(r, Kc), _run(r, Kc, loop=True)
    assert o["kernel"] == "ce_vjp_tri_many" and l["path"] == "loop" and l["kernel"] is None
    (dA, dq, adj), (dA_l, dq_l, adj_l) = o["out"], l["out"]
    assert ((adj & (4 | 8)) == (adj[:1] & (4 | 8))).all()          # flags are the matrix's: the same for every cotangent
    both = (adj == 0) & (adj_l == 0)
    assert (both.mean(axis=1) >= MIN_SHARE).all(), (name, Kc, both.mean(axis=1))
    eA = (np.abs(dA - dA_l).max(axis=2) / (1 + np.abs(dA_l).max(axis=2)))[both]
    eq = (np.abs(dq - dq_l).max(axis=2) / (1 + np.abs(dq_l).max(axis=2)))[both]
    print(f"{name} K={Kc}: against the loop dA {eA.max():.2e} dq {eq.max():.2e}; flagged here {int((adj[0] != 0).sum())}, by the pivoting kernel {int((adj_l[0] != 0).sum())}")
    assert eA.max() < 1e-6 and eq.max() < 1e-6, (name, Kc, eA.max(), eq.max())
    if Kc >= 3:
        un = adj[ZERO_AT] == 0
        assert (dA[ZERO_AT][un] == 0).all() and (dq[ZERO_AT][un] == 0).all()
        e0 = np.abs(dA[0] - dA[Kc - 1]).max(axis=1) / (1 + np.abs(dA[0]).max(axis=1))          # the repeated cotangent, first and last
        print(f"{name} K={Kc}: cotangent 0 against its repeat {e0.max():.2e}")
        assert e0.max() < 1e-6, (name, Kc, e0.max())


@pytest.mark.parametrize("name", ["exp_pow_mixed", "E"])
def test_transpose_identity_against_the_forward_derivative(name):
    """<x-bar_k, dx> + <y-bar_k, dy>  ==  <dA_k, tA_eval> + <dq_k, tq_eval>  per instance and cotangent, against ce_jvp (the TRI forward mode)"""
    r = _point(name)
    eng, (x, y, s) = r["eng"], r["pt"]
    Kc = 3
    _, tA_bm, tq = _tangents(r["tpl"], r["A"].shape[0], seed=K.SHAPES[name][3] + 100)
    dx, dy, ds, st = eng.jvp(r["A_bm"], x, y, s, tA_bm, tq, path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], method="direct")
    assert eng.last_jvp_kernel == "ce_jvp"
    torch.cuda.synchronize()
    dA, dq, adj = _run(r, Kc)["out"]
    xb, yb = cotangents(Kc, r["base_dx"], r["base_dy"])
    st = st.cpu().numpy(); dx, dy, tA, tqn = dx.cpu().numpy(), dy.cpu().numpy(), tA_bm.cpu().numpy(), tq.cpu().numpy().T
    for k in (0, 2):
        both = (st == 0) & (adj[k] == 0)
        assert both.mean() >= MIN_SHARE, (name, k, both.mean())
        lhs = ((xb[k] * dx).sum(axis=1) + (yb[k] * dy).sum(axis=1))[both]
        rhs = ((dA[k] * tA).sum(axis=1) + (dq[k] * tqn).sum(axis=1))[both]
        print(f"{name} k={k}: transpose identity max |lhs - rhs| / (1 + |lhs| + |rhs|) = {(np.abs(lhs - rhs) / (1 + np.abs(lhs) + np.abs(rhs))).max():.2e}, compared {both.mean():.3f}")
        assert (np.abs(lhs - rhs) < 1e-6 * (1 + np.abs(lhs) + np.abs(rhs))).all(), (lhs, rhs)
        assert np.abs(lhs).max() > 1e-3


def test_duplicated_equality_rows_are_flagged_for_every_cotangent_and_resolved():
    """the construction of test_gpu_tri_jvp.py::test_duplicated_equality_rows_are_flagged_and_resolved with K = 3: status 12 for every k on the degenerate instances,
    0 on the others; the degenerate ones within 1e-6 (1 + max |want|) of the oracle's LSQR adjoint under TIGHT_LSQR"""
    from oracle import oracle
    n, cones, B, seed, _ = K.SHAPES["exp_pow_mixed"]
    Kc = 3
    A, b, c = P.generate(n, cones, B, seed=seed)
    deg = np.arange(B) % 2 == 0
    A[deg, 1, :] = A[deg, 0, :]; b[deg, 1] = b[deg, 0]
    ref = oracle.solve_batch(A, b, c, cones, eps=1e-10, max_iters=200000)
    keep = ref["status"] == 1
    assert keep.mean() >= 0.8, keep.mean()
    A, b, c, deg = A[keep], b[keep], c[keep], deg[keep]
    ref = {k: v[keep] for k, v in ref.items()}
    tpl = P.dense_template(n, cones)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    eng = _engine(tpl)
    rng = np.random.default_rng(seed + 12)
    dx = rng.standard_normal((Kc,) + ref["x"].shape); dy = rng.standard_normal((Kc,) + ref["y"].shape)
    dA, dq, adj = eng.vjp_many(torch.from_numpy(A_eval).cuda().t().contiguous(), *(torch.from_numpy(ref[k]).cuda() for k in "xys"), torch.from_numpy(dx).cuda(),
                               torch.from_numpy(dy).cuda(), path="per_instance", lsqr=TIGHT_LSQR, q_eval=torch.from_numpy(q_eval).cuda(), tri_many=True)
    assert eng.last_vjp_many_path == "many" and eng.last_vjp_kernel == "ce_vjp_tri_many"
    torch.cuda.synchronize()
    a, dA = adj.cpu().numpy(), dA.cpu().numpy()
    for k in range(Kc):
        print(f"duplicated rows k={k}: status {a[k].tolist()}")
        assert (a[k][deg] == 12).all() and (a[k][~deg] == 0).all(), (k, a[k])
        g = oracle.adjoint_batch(A[deg], b[deg], c[deg], cones, ref["x"][deg], ref["y"][deg], ref["s"][deg], dx[k][deg], dy[k][deg], mode="lsqr",
                                 lsqr_atol=TIGHT_LSQR[0], lsqr_btol=TIGHT_LSQR[1], lsqr_iter_lim=TIGHT_LSQR[2])
        want = _boundary(tpl, g, n).T
        err = np.abs(dA[k][deg] - want).max()
        print(f"duplicated rows k={k}: {err:.2e} against {1e-6 * (1 + np.abs(want).max()):.2e}")
        assert err < 1e-6 * (1 + np.abs(want).max()), (k, err)


def test_without_the_flag_the_same_engine_runs_the_loop_bit_for_bit():
    r = _point("exp_pow_mixed")
    eng, Kc = r["eng"], 3
    dx, dy = cotangents(Kc, r["base_dx"], r["base_dy"])
    dxt, dyt = torch.from_numpy(dx).cuda(), torch.from_numpy(dy).cuda()
    dA, dq, adj = eng.vjp_many(r["A_bm"], *r["pt"], dxt, dyt, path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"])
    assert eng.last_vjp_many_path == "loop" and eng.last_vjp_kernel is None
    for k in range(Kc):
        a1, q1, s1 = eng.vjp(r["A_bm"], *r["pt"], dxt[k], dyt[k], path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"])
        assert torch.equal(dA[k], a1.t()) and torch.equal(dq[k], q1.t()) and torch.equal(adj[k], s1)
    # and with the flag where the elimination does not run: no q_eval (no re-solve), force_loop -- the loop, as without it
    for kw in (dict(path="per_instance"), dict(path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], force_loop=True)):
        got = eng.vjp_many(r["A_bm"], *r["pt"], dxt, dyt, tri_many=True, **kw)
        assert eng.last_vjp_many_path == "loop" and eng.last_vjp_kernel is None, kw
        ref = eng.vjp_many(r["A_bm"], *r["pt"], dxt, dyt, **kw)
        assert all(torch.equal(u, v) for u, v in zip(got, ref)), kw


def _same_with_and_without(eng, args, **kw):
    a = eng.vjp_many(*args, tri_many=True, **kw)
    pa = (eng.last_vjp_many_path, eng.last_vjp_kernel)
    b = eng.vjp_many(*args, **kw)
    assert pa == (eng.last_vjp_many_path, eng.last_vjp_kernel), pa
    assert len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))
    return pa


def test_the_flag_changes_nothing_on_templates_without_triples():
    from test_gpu_parity import gpu_solve
    rng = np.random.default_rng(5)
    Kc = 2
    # plain cones: ce_vjp_many's one call, as without the flag
    n, cones, B = 8, {"z": 2, "l": 6, "q": [4]}, 8
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=1)
    eng, A_bm, x, y, s, *_ = gpu_solve(tpl, A, b, c, eps=1e-9, max_iters=200000)
    q_t = torch.from_numpy(tpl.values_from_dense(A, b, c)[1]).cuda()
    dx = torch.from_numpy(rng.standard_normal((Kc, B, n))).cuda(); dy = torch.from_numpy(rng.standard_normal((Kc, B, tpl.m))).cuda()
    assert _lib.lib().ce_vjp_tri_many_variant(eng._h) == -1
    assert _same_with_and_without(eng, (A_bm, x, y, s, dx, dy), path="per_instance", lsqr=TIGHT_LSQR, q_eval=q_t) == ("many", "ce_vjp_many")
    # raw ce_vjp_tri_many on it: CE_E_UNSUPPORTED, the reason named, nothing written
    f64 = dict(dtype=torch.float64, device="cuda")
    dA = torch.full((Kc, B, eng.nnz_aug), 7.0, **f64); dq = torch.full((Kc, B, n + 1), 7.0, **f64)
    A_c = A_bm.contiguous()
    rc = _lib.lib().ce_vjp_tri_many(eng._h, B, Kc, A_c.data_ptr(), eng.nnz_aug, q_t.data_ptr(), q_t.stride(0), q_t.stride(1), x.data_ptr(), y.data_ptr(), s.data_ptr(),
                                    dx.data_ptr(), None, dA.data_ptr(), dq.data_ptr(), None, None)
    msg = (_lib.lib().ce_last_error() or b"").decode()
    torch.cuda.synchronize()
    assert rc == -2 and "ce_vjp_tri_many" in msg and "no exponential / power cone" in msg, (rc, msg)
    assert (dA == 7.0).all() and (dq == 7.0).all()
    # a PSD template: the loop
    n, cones, B = 4, {"z": 1, "s": [3]}, 4
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=2)
    eng, A_bm, x, y, s, *_ = gpu_solve(tpl, A, b, c, eps=1e-9, max_iters=200000)
    q_t = torch.from_numpy(tpl.values_from_dense(A, b, c)[1]).cuda()
    dx = torch.from_numpy(rng.standard_normal((Kc, B, n))).cuda(); dy = torch.from_numpy(rng.standard_normal((Kc, B, tpl.m))).cuda()
    assert _lib.lib().ce_vjp_tri_many_variant(eng._h) == -1
    assert _same_with_and_without(eng, (A_bm, x, y, s, dx, dy), path="per_instance", lsqr=TIGHT_LSQR, q_eval=q_t) == ("loop", None)


def test_the_flag_changes_nothing_on_a_native_quadratic_objective():
    import qp_ns_kit as Q
    from test_quad_objective import _upper_structure
    from cvxpylayers_amd.interfaces.mi355_if import make_settings
    n, cones, A, b, c, Pm = Q.instance("small_mixed")
    tpl = P.dense_template(n, cones)
    struct = _upper_structure(n)
    eng = Q.qp_engine(tpl, struct)
    assert eng.qp_native and _lib.lib().ce_vjp_tri_many_variant(eng._h) == -1
    A_bm, q_t, P_bm = Q.device_values(tpl, A, b, c, Pm, struct)
    x, y, s, *_ = eng.solve(A_bm, q_t, make_settings(dict(eps=1e-9, max_iters=200000, acceleration_lookback=0)), P_bm=P_bm)
    B, Kc = A.shape[0], 2
    rng = np.random.default_rng(3)
    dx = torch.from_numpy(rng.standard_normal((Kc, B, n))).cuda(); dy = torch.from_numpy(rng.standard_normal((Kc, B, tpl.m))).cuda()
    assert _same_with_and_without(eng, (A_bm, x, y, s, dx, dy), path="per_instance", q_eval=q_t, P_bm=P_bm) == ("loop", None)


def test_a_null_dy_is_the_zero_cotangent():
    r = _point("exp_small")
    eng = r["eng"]
    dx, dy = cotangents(3, r["base_dx"], r["base_dy"])
    dxt = torch.from_numpy(dx).cuda()
    a = eng.vjp_many(r["A_bm"], *r["pt"], dxt, None, path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], tri_many=True)
    assert eng.last_vjp_kernel == "ce_vjp_tri_many"
    b = eng.vjp_many(r["A_bm"], *r["pt"], dxt, torch.zeros_like(torch.from_numpy(dy)).cuda(), path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], tri_many=True)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_empty_batches_and_no_cotangent_return_empty_tensors():
    r = _point("exp_small")
    eng, B, n, m = r["eng"], r["A"].shape[0], r["n"], r["tpl"].m
    z = torch.zeros((0, B, n), dtype=torch.float64, device="cuda")
    dA, dq, adj = eng.vjp_many(r["A_bm"], *r["pt"], z, None, path="per_instance", q_eval=r["q_t"], tri_many=True)
    assert dA.shape == (0, B, eng.nnz_aug) and dq.shape == (0, B, n + 1) and adj.shape == (0, B)
    e = torch.zeros((0, m), dtype=torch.float64, device="cuda")
    dA, dq, adj = eng.vjp_many(r["A_bm"][:0], e[:, :n], e, e, torch.zeros((2, 0, n), dtype=torch.float64, device="cuda"), None, path="per_instance", q_eval=r["q_t"][:, :0],
                               tri_many=True)
    assert dA.shape == (2, 0, eng.nnz_aug) and dq.shape == (2, 0, n + 1) and adj.shape == (2, 0)

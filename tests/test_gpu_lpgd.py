"""solver_args mode="lpgd" / "lpgd_left" / "lpgd_right" through the plugin (interfaces/lpgd.py behind mi355_if.py) against oracle LPGD (lpgd_kit.py): the same
perturbed programs solved by the oracle, the same differences in numpy.

The bound is derived (lpgd_kit.py): G is bilinear in the point, so with e_a, e_b the measured engine-versus-oracle distances (max norm over x and y) of the two
points a difference is formed from, an entry of the gradient differs by at most (|x|_inf + |y|_inf + 1) (e_a + e_b) / delta.  For the one-sided modes that is the
issue's (|x|_inf + |y|_inf + 1) (delta_0 + delta_tau) / tau; for the central one (e_+ + e_-) / (2 tau) asks more than it.  The distances themselves are held to the
bound of tests/test_gpu_parity.py at the same eps: max(1e-6, 20 eps) (1 + |want|_inf).
Known answers with no oracle: a linear objective over the simplex, where LPGD returns differences of vertices and the adjoint returns zeros."""
import functools

import numpy as np
import pytest
import torch

import lpgd_kit as lk
import value_kit as vk
from cvxpylayers_amd import problems as P

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
EPS = 1e-9
ARGS = {"eps": EPS, "max_iters": 200000, "acceleration_lookback": 0}          # (the oracle's plain iteration, as the parity tests run it)
PARITY_TOL = max(1e-6, 20 * EPS)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ctx(tpl, struct=None, options=ARGS):
    from cvxpylayers_amd.interfaces.mi355_if import MI355_ctx
    return MI355_ctx(struct, tpl.problem_data_index, tpl.cones, options=dict(options))


def _p_values(Pm, struct):
    idx, ptr, _ = struct
    return Pm[:, idx, np.repeat(np.arange(Pm.shape[-1]), np.diff(ptr))]          # (B, nnz_p)


def _run(ctx, tpl, A, b, c, dx, dy, args, Pm=None, struct=None, warm_start=None, batch_major_storage=False):
    """one forward and one backward of loss = <dx, primal> + <dy, dual> through the plugin: numpy dA (nnz_aug, B), dq (n+1, B), dP (nnz_p, B) or None, the
    outputs and info.  dy = None: the loss does not touch the duals."""
    from cvxpylayers_amd.interfaces.mi355_if import _CvxpyLayer
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    A_t, q_t = _cuda(A_eval), _cuda(q_eval)
    if batch_major_storage:
        A_t = A_t.t().contiguous().t()
    A_t.requires_grad_(); q_t.requires_grad_()
    P_t = _cuda(_p_values(Pm, struct).T).requires_grad_() if Pm is not None else None
    primal, dual, info, _ = _CvxpyLayer.apply(P_t, q_t, A_t, ctx, args, True, warm_start)
    loss = (primal * _cuda(dx)).sum()
    if dy is not None:
        loss = loss + (dual * _cuda(dy)).sum()
    loss.backward()
    torch.cuda.synchronize()
    out = dict(dA=A_t.grad.cpu().numpy(), dq=q_t.grad.cpu().numpy(), dP=P_t.grad.cpu().numpy() if P_t is not None else None,
               x=primal.detach().cpu().numpy(), y=dual.detach().cpu().numpy(), info=info)
    return out


def _fold_P(dP_dense, struct):
    """dense 1/2 (x x^T) differences -> the one-triangle structure's entries (an off-diagonal entry stands for both matrix entries)"""
    idx, ptr, _ = struct
    cols = np.repeat(np.arange(dP_dense.shape[-1]), np.diff(ptr))
    return np.where(idx == cols, dP_dense[:, idx, cols], dP_dense[:, idx, cols] + dP_dense[:, cols, idx]).T          # (nnz_p, B)


@functools.lru_cache(maxsize=None)
def _oracle_base(name):
    """the oracle's base point of a layer case: computed once, shared, never changed"""
    from oracle import oracle
    cs = lk.layer_case(name)
    base = oracle.solve_batch(cs["A"], cs["b"], cs["c"], cs["cones"], P=cs["P"], eps=EPS, max_iters=200000)
    assert (base["status"] == 1).all()
    return cs, base


def _dist(got_x, got_y, ref):
    return np.maximum(np.abs(got_x - ref["x"]).max(axis=1), np.abs(got_y - ref["y"]).max(axis=1))


def _check_case(name, mode, rho, monkeypatch):
    from cvxpylayers_amd.interfaces.lpgd import perturbed_points
    cs, base = _oracle_base(name)
    tpl, tau = cs["tpl"], lk.LAYER_TAU
    if cs["shared"]:
        monkeypatch.setenv("CE_CONST_A", "1")
    ctx = _ctx(tpl, cs["struct"])
    args = {"mode": mode, "lpgd_tau": tau, "lpgd_rho": rho}
    got = _run(ctx, tpl, cs["A"], cs["b"], cs["c"], cs["dx"], cs["dy"], args, Pm=cs["P"], struct=cs["struct"])
    eng = ctx.engine(DEV)
    adj = got["info"]["adjoint"]
    assert adj["path"] == mode and adj["tau"] == tau and adj["rho"] == rho
    assert (adj["status"].cpu().numpy() == 0).all() and tuple(adj["lpgd_iters"].shape) == (len(lk.sides(mode)), cs["A"].shape[0])
    assert eng.last_path == ("const_a" if cs["shared"] else "per_instance")
    if cs["P"] is not None:
        assert eng.qp_native
    # oracle LPGD on the same data
    want = lk.oracle_lpgd(cs["A"], cs["b"], cs["c"], cs["cones"], cs["dx"], cs["dy"], tau, rho, mode, P=cs["P"], base=base, eps=EPS, max_iters=200000)
    o_pts = want["points"]["pts"]
    assert all((r["status"] == 1).all() for r in o_pts.values())
    # the engine's own points: the base point of the forward above and the perturbed points, re-computed by the calls the backward makes
    x0, y0, s0 = eng._last_solution
    from cvxpylayers_amd.interfaces.mi355_if import make_settings
    A_eval, q_eval = tpl.values_from_dense(cs["A"], cs["b"], cs["c"])
    P_bm = _cuda(_p_values(cs["P"], cs["struct"])) if cs["P"] is not None else None
    e_pts, _, flags, bad = perturbed_points(eng, (mode, tau, rho), make_settings(dict(ARGS)), eng.last_path, _cuda(A_eval.T), _cuda(q_eval), P_bm,
                                            x0, y0, s0, _cuda(cs["dx"]), _cuda(cs["dy"]))
    assert not bad.any() and (flags == 0).all()
    e0 = _dist(x0.cpu().numpy(), y0.cpu().numpy(), base)
    e = {sg: _dist(e_pts[sg][0].cpu().numpy(), e_pts[sg][1].cpu().numpy(), o_pts[sg]) for sg in o_pts}
    e_xy = {sg: (e_pts[sg][0].cpu().numpy(), e_pts[sg][1].cpu().numpy()) for sg in o_pts}
    for what, (gx, gy), ref in [("base", (x0.cpu().numpy(), y0.cpu().numpy()), base)] + [(f"side {sg:+.0f}", e_xy[sg], o_pts[sg]) for sg in e]:
        rel = np.maximum(np.abs(gx - ref["x"]).max(axis=1) / (1 + np.abs(ref["x"]).max(axis=1)), np.abs(gy - ref["y"]).max(axis=1) / (1 + np.abs(ref["y"]).max(axis=1)))
        print(f"{name} {mode} rho={rho}: engine vs oracle at the {what} point: {rel.max():.2e} (parity bound {PARITY_TOL:.0e})")
        assert rel.max() < PARITY_TOL, (what, rel.max())
    ea, eb, delta = {"lpgd_right": (e0, e.get(1.0), tau), "lpgd_left": (e.get(-1.0), e0, tau), "lpgd": (e.get(-1.0), e.get(1.0), 2 * tau)}[mode]
    refs = [base] + list(o_pts.values())
    size = np.max([np.abs(r["x"]).max(axis=1) for r in refs], axis=0) + np.max([np.abs(r["y"]).max(axis=1) for r in refs], axis=0) + 1.0
    bound = size * (ea + eb) / delta
    w_dA, w_dq = lk.to_boundary(tpl, want)
    checks = [("dA", got["dA"], w_dA), ("dq", got["dq"], w_dq)]
    if cs["P"] is not None:
        checks.append(("dP", got["dP"], _fold_P(want["dP"], cs["struct"])))
    for key, g_, w_ in checks:
        err = np.abs(g_ - w_).max(axis=0)
        print(f"{name} {mode} rho={rho} {key}: max error / bound = {(err / bound).max():.3f} (errors up to {err.max():.2e}, gradients up to {np.abs(w_).max():.2e})")
        assert (err <= bound).all(), (key, (err / bound).max())
    assert np.abs(w_dq).max() > 1e-3


@pytest.mark.parametrize("mode", lk.MODES)
@pytest.mark.parametrize("name", lk.LAYER_CASES)
def test_layer_gradients_equal_oracle_lpgd(name, mode, monkeypatch):
    _check_case(name, mode, 0.0, monkeypatch)


@pytest.mark.parametrize("name", ["qp_native", "soc"])
def test_layer_gradients_with_a_proximal_weight(name, monkeypatch):
    """rho > 0: on the QP-native template P + rho I is built by ce_lpgd_perturb; on the second-order-cone template (linear objective) a sibling engine with a
    diagonal P structure solves the perturbed programs"""
    _check_case(name, "lpgd", 0.5, monkeypatch)
    _check_case(name, "lpgd_right", 0.5, monkeypatch)


# ------------------------------------------------------------------------------------------------ known answers over the simplex
SIMPLEX_EPS = 1e-8
SIMPLEX_ARGS = {"eps_abs": SIMPLEX_EPS, "eps_rel": 0.0, "max_iters": 200000, "acceleration_lookback": 0}          # eps_solve: a purely absolute stopping tolerance


def _simplex():
    n, B, tau = 6, 64, 0.1
    A, b, cones = lk.simplex_program(n, B)
    c, dx = lk.simplex_draw(n, B, tau, seed=23)
    return n, B, tau, A, b, c, dx, P.dense_template(n, cones, pattern=(A[0] != 0), b_pattern=(b[0] != 0))


def test_simplex_lpgd_returns_differences_of_vertices_where_the_adjoint_returns_zeros():
    """min c^T x over {x >= 0, 1^T x = 1}, n = 6, B = 64; c and dx drawn by seeded rejection (the two smallest entries of c, c + tau dx, c - tau dx at least 0.05
    apart).  rho = 0:  dq = (e_j+ - e_j0) / tau for lpgd_right, (e_j+ - e_j-) / (2 tau) for lpgd, within 2 eps_solve / tau; the default adjoint gives zeros at
    that resolution.  (The seed was fixed on the CPU: the oracle's own answers are within 0.78 / 0.38 of the bound for the two modes.)"""
    n, B, tau, A, b, c, dx, tpl = _simplex()
    E = np.eye(n)
    j0, jp, jm = c.argmin(axis=1), (c + tau * dx).argmin(axis=1), (c - tau * dx).argmin(axis=1)
    flipped = jp != j0
    assert 5 <= flipped.sum() <= B - 5
    tol = 2 * SIMPLEX_EPS / tau
    for mode, want in (("lpgd_right", (E[jp] - E[j0]) / tau), ("lpgd", (E[jp] - E[jm]) / (2 * tau))):
        got = _run(_ctx(tpl, options=SIMPLEX_ARGS), tpl, A, b, c, dx, None, {"mode": mode, "lpgd_tau": tau})
        err = np.abs(got["dq"][:n].T - want).max(axis=1)
        print(f"{mode}: max |dq - want| = {err.max():.2e}, bound {tol:.1e}; {int(flipped.sum())} of {B} instances flip vertex")
        assert (got["info"]["adjoint"]["status"].cpu().numpy() == 0).all()
        assert (err <= tol).all(), err.max()
        if mode == "lpgd_right":
            assert np.abs(got["dq"][:n].T[~flipped]).max() <= tol          # the unflipped instances: nothing moved
            assert np.allclose(np.abs(got["dq"][:n].T[flipped]).max(axis=1), 1 / tau, atol=tol)
    # the default adjoint on the same batch: the solution map is piecewise constant, its derivative is zero
    got = _run(_ctx(tpl, options=SIMPLEX_ARGS), tpl, A, b, c, dx, None, {})
    print(f"default adjoint: max |dq| = {np.abs(got['dq'][:n]).max():.2e}")
    assert np.abs(got["dq"][:n]).max() <= tol


def test_simplex_with_a_proximal_weight_projects_onto_the_simplex():
    """rho > 0: the perturbed program is min (c + tau dx - rho x*)^T x + rho / 2 |x|^2 over the simplex, so x+ is the Euclidean projection of x* - (c + tau dx) / rho
    (sort-based closed form); lpgd_right returns (x+ - x*) / tau, within 2 eps_solve / tau (the oracle's own answer: 0.73 of it)"""
    n, B, tau, A, b, c, dx, tpl = _simplex()
    rho = 0.5
    E = np.eye(n)
    j0 = c.argmin(axis=1)
    got = _run(_ctx(tpl, options=SIMPLEX_ARGS), tpl, A, b, c, dx, None, {"mode": "lpgd_right", "lpgd_tau": tau, "lpgd_rho": rho})
    want = (lk.simplex_projection(E[j0] - (c + tau * dx) / rho) - E[j0]) / tau
    err = np.abs(got["dq"][:n].T - want).max()
    print(f"rho = {rho}: max |dq - want| = {err:.2e}, bound {2 * SIMPLEX_EPS / tau:.1e}")
    assert err <= 2 * SIMPLEX_EPS / tau
    inside = (lk.simplex_projection(E[j0] - (c + tau * dx) / rho) > 1e-3).sum(axis=1) >= 2
    assert inside.sum() >= 5          # (with the proximal term the perturbed solution leaves the vertices: here it lies inside a face)


# ------------------------------------------------------------------------------------------------ cotangents and statuses
def test_zero_cotangent_instances_get_exact_zeros():
    cs, _ = _oracle_base("soc")
    dx, dy = cs["dx"].copy(), cs["dy"].copy()
    dx[[0, 5]] = 0.0; dy[[0, 5]] = 0.0
    for mode in ("lpgd", "lpgd_right"):
        got = _run(_ctx(cs["tpl"]), cs["tpl"], cs["A"], cs["b"], cs["c"], dx, dy, {"mode": mode, "lpgd_tau": 0.05})
        assert (got["dA"][:, [0, 5]] == 0).all() and (got["dq"][:, [0, 5]] == 0).all()
        assert np.abs(got["dA"][:, 1]).max() > 1e-3 and (got["info"]["adjoint"]["status"].cpu().numpy() == 0).all()
    # the loss touches the primal variables only: dy = NULL inside, the same gradients as an explicit zero cotangent on the duals
    a = _run(_ctx(cs["tpl"]), cs["tpl"], cs["A"], cs["b"], cs["c"], dx, None, {"mode": "lpgd", "lpgd_tau": 0.05})
    z = _run(_ctx(cs["tpl"]), cs["tpl"], cs["A"], cs["b"], cs["c"], dx, np.zeros_like(dy), {"mode": "lpgd", "lpgd_tau": 0.05})
    assert np.array_equal(a["dA"], z["dA"]) and np.array_equal(a["dq"], z["dq"])


def test_a_dual_cotangent_on_a_row_without_a_b_slot_is_dropped_and_reported():
    n, cones, B, seed, _ = vk.KERNEL_SHAPES["sparse_b5"]
    A, b, c, pattern, b_pattern = vk.sparse_instance(n, cones, B, seed)
    tpl = P.dense_template(n, cones, pattern=pattern, b_pattern=b_pattern)
    row = int(np.nonzero(~b_pattern)[0][0])
    rng = np.random.default_rng(7)
    dx, dy = rng.standard_normal((B, n)), rng.standard_normal((B, tpl.m)) * b_pattern[None]
    empty = np.nonzero(~pattern.any(axis=0))[0]
    dx[:, empty] = 0.0          # (a variable in no constraint: its cost must stay zero, or the perturbed program is unbounded -- used below)
    dy_bad = dy.copy(); dy_bad[1, row] = 0.7
    args = {"mode": "lpgd", "lpgd_tau": 0.05}
    clean = _run(_ctx(tpl), tpl, A, b, c, dx, dy, args)
    got = _run(_ctx(tpl), tpl, A, b, c, dx, dy_bad, args)
    status = got["info"]["adjoint"]["status"].cpu().numpy()
    assert status[1] == 32 and (np.delete(status, 1) == 0).all() and (clean["info"]["adjoint"]["status"].cpu().numpy() == 0).all()
    assert np.array_equal(got["dA"], clean["dA"]) and np.array_equal(got["dq"], clean["dq"])
    # a perturbed program without a solution (a cost on the variable no constraint holds: unbounded): bit 16, exact zeros, the other instances unchanged
    dx_bad = dx.copy(); dx_bad[2, empty[0]] = 1.0
    got = _run(_ctx(tpl), tpl, A, b, c, dx_bad, dy, args)
    status = got["info"]["adjoint"]["status"].cpu().numpy()
    assert status[2] == 16 and (np.delete(status, 2) == 0).all(), status
    keep = np.arange(B) != 2
    for key in ("dA", "dq"):
        assert (got[key][:, 2] == 0).all() and np.array_equal(got[key][:, keep], clean[key][:, keep]), key


def test_a_failed_instance_gets_exact_zeros_and_the_others_do_not_notice():
    """raise_on_error=False with one infeasible instance (the construction of test_gpu_value.py::test_a_masked_instance_returns_nan_and_contributes_no_gradient)"""
    n, cones = lk.SOC_SHAPE
    B, bad = 6, 2
    A, b, c = P.generate(n, cones, B, seed=33)
    A[bad, 3] = -A[bad, 2]; b[bad, 2] = -1.0; b[bad, 3] = -1.0
    tpl = P.dense_template(n, cones)
    rng = np.random.default_rng(8)
    dx, dy = rng.standard_normal((B, n)), rng.standard_normal((B, tpl.m))
    args = {"mode": "lpgd_right", "lpgd_tau": 0.05, "raise_on_error": False}
    got = _run(_ctx(tpl, options={"eps": 1e-8, "max_iters": 20000}), tpl, A, b, c, dx, dy, args)
    assert got["info"]["status"].cpu().numpy()[bad] < 0 and np.isnan(got["x"][bad]).all()
    keep = np.arange(B) != bad
    rest = _run(_ctx(tpl, options={"eps": 1e-8, "max_iters": 20000}), tpl, A[keep], b[keep], c[keep], dx[keep], dy[keep], args)
    for key in ("dA", "dq"):
        assert np.isfinite(got[key]).all() and (got[key][:, bad] == 0).all(), key
        assert np.array_equal(got[key][:, keep], rest[key]), key


# ------------------------------------------------------------------------------------------------ leaving no trace
def test_a_forward_after_an_lpgd_backward_returns_what_it_returns_without_it():
    """forward, backward(lpgd), forward == forward, forward bit for bit, the second forward warm-started from the layer's memory"""
    from cvxpylayers_amd.interfaces.mi355_if import _CvxpyLayer
    cs, _ = _oracle_base("soc")
    tpl = cs["tpl"]
    A_eval, q_eval = tpl.values_from_dense(cs["A"], cs["b"], cs["c"])
    A2, q2 = tpl.values_from_dense(cs["A"], cs["b"] + 0.01, cs["c"] * 1.01)          # the second forward: nearby data, so the warm start matters
    outs = []
    for with_backward in (True, False):
        ctx = _ctx(tpl, options={"eps": 1e-8, "max_iters": 100000})          # (default acceleration, dispatch history on)
        args = {"mode": "lpgd", "lpgd_tau": 0.05}
        if with_backward:
            _run(ctx, tpl, cs["A"], cs["b"], cs["c"], cs["dx"], cs["dy"], args)
        else:
            _CvxpyLayer.apply(None, _cuda(q_eval), _cuda(A_eval), ctx, args, True, None)
        primal, dual, info, _ = _CvxpyLayer.apply(None, _cuda(q2), _cuda(A2), ctx, args, True, True)
        torch.cuda.synchronize()
        outs.append((primal.clone(), dual.clone(), info["iters"].clone(), info["status"].clone()))
    for a, b_ in zip(*outs):
        assert torch.equal(a, b_)


def test_a_default_mode_backward_after_an_lpgd_backward_returns_what_it_returns_alone():
    from cvxpylayers_amd.interfaces.mi355_if import _CvxpyLayer
    cs, _ = _oracle_base("soc")
    tpl = cs["tpl"]
    A_eval, q_eval = tpl.values_from_dense(cs["A"], cs["b"], cs["c"])
    A2, q2 = tpl.values_from_dense(cs["A"][:8], cs["b"][:8] + 0.01, cs["c"][:8])
    wx, wy = _cuda(cs["dx"]), _cuda(cs["dy"])
    grads = []
    for with_lpgd in (True, False):
        ctx = _ctx(tpl, options={"eps": 1e-8, "max_iters": 100000})
        if with_lpgd:
            A1, q1 = _cuda(A_eval).requires_grad_(), _cuda(q_eval).requires_grad_()
            p1, d1, _, _ = _CvxpyLayer.apply(None, q1, A1, ctx, {"mode": "lpgd_right", "lpgd_tau": 0.05}, True, None)
        At, qt = _cuda(A2).requires_grad_(), _cuda(q2).requires_grad_()
        p2, d2, info2, _ = _CvxpyLayer.apply(None, qt, At, ctx, {}, True, None)
        if with_lpgd:
            ((p1 * wx).sum() + (d1 * wy).sum()).backward()
        ((p2 * wx[:8]).sum() + (d2 * wy[:8]).sum()).backward()
        torch.cuda.synchronize()
        grads.append((At.grad.clone(), qt.grad.clone(), info2["adjoint"]["status"].clone()))
        assert info2["adjoint"]["path"] == "per_instance"
    for a, b_ in zip(*grads):
        assert torch.equal(a, b_)


# ------------------------------------------------------------------------------------------------ refusals
def test_rho_on_a_P_structure_without_the_full_diagonal_is_refused():
    n, cones, B = 6, {"z": 2, "l": 4, "q": []}, 4
    A, b, c = P.generate(n, cones, B, seed=4)
    tpl = P.dense_template(n, cones)
    struct = (np.arange(1, n, dtype=np.int32), np.concatenate([[0], np.arange(n)]).astype(np.int32), (n, n))          # a diagonal P without the (0, 0) entry
    Pm = np.zeros((B, n, n)); Pm[:, np.arange(1, n), np.arange(1, n)] = 1.0
    dx = np.ones((B, n))
    ctx = _ctx(tpl, struct, options={"eps": 1e-8})
    got = _run(ctx, tpl, A, b, c, dx, None, {"mode": "lpgd", "lpgd_tau": 0.05}, Pm=Pm, struct=struct)          # rho = 0 is served
    assert ctx.engine(DEV).qp_native and np.isfinite(got["dP"]).all()
    with pytest.raises(ValueError, match="full diagonal"):
        _run(ctx, tpl, A, b, c, dx, None, {"mode": "lpgd", "lpgd_tau": 0.05, "lpgd_rho": 0.5}, Pm=Pm, struct=struct)


def test_rho_on_a_template_whose_sibling_cannot_run_P_inside_the_kernels_is_refused():
    """ce_plan.h: P runs inside the kernels for plain cones only, so a PSD block is the cheapest trigger of ce_qp_native() == 0"""
    cs, _ = _oracle_base("psd")
    ctx = _ctx(cs["tpl"])
    with pytest.raises(ValueError, match="lpgd_rho=0"):
        _run(ctx, cs["tpl"], cs["A"], cs["b"], cs["c"], cs["dx"], cs["dy"], {"mode": "lpgd", "lpgd_tau": 0.05, "lpgd_rho": 0.5})


# ------------------------------------------------------------------------------------------------ the handle's retained forward state, arguments, empty batches, warnings
def test_a_transient_solve_leaves_the_retained_forward_inputs_alone():
    """ce_solve retains its batch-major A for ce_vjp(A_vals = NULL).  solve on data 1, a solve on OTHER data, then ce_vjp(NULL) with data 1's point: under
    ce_set_transient_solve the gradients are those of the run without the second solve, bit for bit; an ordinary second solve redirects them (the hazard)."""
    import ctypes as C
    from cvxpylayers_amd import _lib
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine, make_settings
    cs, _ = _oracle_base("soc")
    tpl = cs["tpl"]
    B, K, n = cs["A"].shape[0], tpl.nnz_aug, tpl.n
    A1, q1 = tpl.values_from_dense(cs["A"], cs["b"], cs["c"])
    A2, q2 = tpl.values_from_dense(1.5 * cs["A"], cs["b"] + 0.3, cs["c"])
    dx, dy = _cuda(cs["dx"]), _cuda(cs["dy"])

    def run(second):
        eng = ConeEngine(tpl.indices, tpl.indptr, n, tpl.m, tpl.cones, DEV)
        eng.set_dispatch_history(True)
        st = make_settings(dict(eps=1e-8, max_iters=100000))
        A_bm1, A_bm2 = _cuda(A1.T), _cuda(A2.T)
        x, y, s, *_ = eng.solve(A_bm1, _cuda(q1), st)
        if second == "transient":
            eng.solve_transient(A_bm2, _cuda(q2), st)
        elif second == "ordinary":
            eng.solve(A_bm2, _cuda(q2), st)
        dA = torch.empty((B, K), dtype=torch.float64, device=DEV); dq = torch.empty((n + 1, B), dtype=torch.float64, device=DEV)
        adj = torch.empty((B,), dtype=torch.int32, device=DEV)
        rc = _lib.lib().ce_vjp(eng._h, B, None, 1, K, None, 0, 0, x.data_ptr(), y.data_ptr(), s.data_ptr(), dx.data_ptr(), dy.data_ptr(),
                               dA.data_ptr(), 1, K, dq.data_ptr(), B, 1, adj.data_ptr(), eng._stream())
        _lib.check(rc, "ce_vjp")
        torch.cuda.synchronize()
        return dA, dq, adj
    alone, transient, ordinary = run(None), run("transient"), run("ordinary")
    for a, b_ in zip(alone, transient):
        assert torch.equal(a, b_)
    assert not torch.equal(alone[0], ordinary[0])          # (without the flag the adjoint reads the second solve's data)
    # a transient solve takes batch-major values only: the layout workspace may hold the retained inputs
    eng = ConeEngine(tpl.indices, tpl.indptr, n, tpl.m, tpl.cones, DEV)
    st = make_settings(dict(eps=1e-8))
    out = [torch.empty((B, k), dtype=torch.float64, device=DEV) for k in (n, tpl.m, tpl.m)]
    it, stt = (torch.empty((B,), dtype=torch.int32, device=DEV) for _ in range(2))
    A_min, q_t = _cuda(A1), _cuda(q1)
    L = _lib.lib()
    assert L.ce_set_transient_solve(eng._h, 1) == 0
    assert L.ce_solve(eng._h, B, A_min.data_ptr(), B, 1, q_t.data_ptr(), B, 1, C.byref(st), *(t.data_ptr() for t in out), it.data_ptr(), stt.data_ptr(), None, eng._stream()) == -1
    assert L.ce_set_transient_solve(eng._h, 0) == 0


def test_bad_lpgd_arguments_raise_before_the_forward_has_side_effects():
    cs, _ = _oracle_base("soc")
    ctx = _ctx(cs["tpl"])
    for bad in ({"lpgd_tau": 0.0}, {"lpgd_rho": -1.0}, {"lpgd_tau": "0.1"}):
        with pytest.raises(ValueError, match=next(iter(bad))):
            _run(ctx, cs["tpl"], cs["A"], cs["b"], cs["c"], cs["dx"], cs["dy"], {"mode": "lpgd", **bad})
    eng = ctx.engine(DEV)
    assert eng._last_solution is None and eng.last_path is None          # nothing was solved, nothing remembered


def test_an_empty_batch_goes_through_the_lpgd_backward():
    cs, _ = _oracle_base("soc")
    tpl = cs["tpl"]
    got = _run(_ctx(tpl), tpl, cs["A"][:0], cs["b"][:0], cs["c"][:0], cs["dx"][:0], cs["dy"][:0], {"mode": "lpgd", "lpgd_tau": 0.05})
    assert got["dA"].shape == (tpl.nnz_aug, 0) and got["dq"].shape == (tpl.n + 1, 0)


def test_the_next_forward_reports_lpgd_flags_under_their_own_causes():
    """bits 16 / 32 of an LPGD backward reach the one warning the next forward gives, and that warning names their causes, not a degenerate active set"""
    import warnings
    from cvxpylayers_amd.interfaces.mi355_if import _CvxpyLayer
    n, cones, B, seed, _ = vk.KERNEL_SHAPES["sparse_b5"]
    A, b, c, pattern, b_pattern = vk.sparse_instance(n, cones, B, seed)
    tpl = P.dense_template(n, cones, pattern=pattern, b_pattern=b_pattern)
    rng = np.random.default_rng(7)
    dx, dy = rng.standard_normal((B, n)), rng.standard_normal((B, tpl.m)) * b_pattern[None]
    dx[:, ~pattern.any(axis=0)] = 0.0
    dy[1, int(np.nonzero(~b_pattern)[0][0])] = 0.7
    ctx = _ctx(tpl)
    got = _run(ctx, tpl, A, b, c, dx, dy, {"mode": "lpgd_right", "lpgd_tau": 0.05})
    assert got["info"]["adjoint"]["status"].cpu().numpy().tolist() == [0, 32, 0, 0, 0]
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        _CvxpyLayer.apply(None, _cuda(q_eval), _cuda(A_eval), ctx, {}, False, None)
    said = [str(x.message) for x in w if "backward" in str(x.message)]
    assert len(said) == 1 and "MI355 LPGD backward: 1 of 5" in said[0] and "dropped" in said[0] and "degenerate" not in said[0], said

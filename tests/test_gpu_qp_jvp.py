"""The forward-mode derivative of templates whose quadratic objective runs inside the kernels: k_backward_ns<..., FWD, QP> behind ce_jvp_qp,
ConeEngine.jvp(method="direct", P_bm=, tP_bm=), solver_args jvp_mode="direct" on the native-QP route.  The search-free null-space elimination with the reduced
Hessian Z^T (H + P) Z; no LSQR runs behind it.  Checked, at the oracle's eps = 1e-10 point and on the instances with status 0 on both sides (>= 80 % of a batch), against
  * the transpose identity  <x-bar, dx> + <y-bar, dy> = <dA, tA> + <dq, tq> + <dP, tP>  with ConeEngine.vjp(P_bm=) -- the pivoting kernel k_backward_rt, another
    algorithm -- and with the oracle's dense QP adjoint itself; tolerance 1e-6 (1 + |lhs| + |rhs|) (test_gpu_jvp_direct.py);
  * the dense numpy solve of  [[P, A^T D], [A, D - I]] (d_x, d_v) = -(g_x, g_y)  (qp_ns_kit.py): max < 1e-5, median < 1e-8 of the per-instance relative error;
  * central differences of the GPU solve (step and bound of test_gpu_jvp_direct.py);
  * null tangents, flagged instances (status 4, no bit 8, no iterations, finite), the plugin and the frontend under torch.autograd.forward_ad.
Shapes: qp_ns_kit.SHAPES (+ P of rank n / 2), the config-2 box QP (row 1 of CE_NS_VARIANTS, multi-wave row elimination when more than 24 bounds are active),
n = 80 on row 2 (512 threads), p = n equalities (nothing left to sweep), SOC only (no zero-cone row), a box that is nowhere active (H = 0)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import qp_ns_kit as K
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from test_gpu_jvp import _engine
from test_quad_objective import _p_values, _upper_structure

pytestmark = pytest.mark.gpu

_CACHE: dict = {}
CASES = list(K.SHAPES) + [s + "_rank_half" for s in K.RANK_HALF] + ["box_qp", "inactive_box"]
EXPECTED_ROW = {"box_qp": 1, "metric": 1, "metric_rank_half": 1, "row2_n80": 2, "small_mixed": 0}


def _case(name):
    """problem, engine, device values, the oracle's eps = 1e-10 point, tangents (dense and as the boundary takes them): computed once, shared, not changed.
    ragged_cones runs on a full symmetric structure, every other case on the upper triangle."""
    if name in _CACHE:
        return _CACHE[name]
    from oracle import oracle
    if name == "box_qp":
        cones, A, b, c, Pm, tpl = K.box_qp()
    elif name == "inactive_box":
        cones, A, b, c, Pm, tpl = K.inactive_box()
    else:
        base = name[:-len("_rank_half")] if name.endswith("_rank_half") else name
        n, cones, A, b, c, Pm = K.instance(base, rank_half=name.endswith("_rank_half"))
        tpl = P.dense_template(n, cones)
    n, m, B = tpl.n, tpl.m, A.shape[0]
    struct = K.full_structure(n) if name == "ragged_cones" else _upper_structure(n)
    ref = oracle.solve_batch(A, b, c, cones, P=Pm, eps=1e-10, max_iters=200000)
    eng = K.qp_engine(tpl, struct)
    A_bm, q_t, P_bm = K.device_values(tpl, A, b, c, Pm, struct)
    rng = np.random.default_rng(100 + len(name))
    tA = rng.standard_normal(A.shape) * (A[:1] != 0 if name in ("box_qp", "inactive_box") else 1.0)          # (tangents live on the template's pattern)
    tb, tc, tP = rng.standard_normal(b.shape), rng.standard_normal(c.shape), K.sym_tangent(B, n, 3)
    tA_eval, tq_eval = tpl.values_from_dense(tA, tb, tc)
    r = dict(name=name, tpl=tpl, cones=cones, A=A, b=b, c=c, Pm=Pm, struct=struct, ref=ref, eng=eng, A_bm=A_bm, q_t=q_t, P_bm=P_bm,
             pt=tuple(torch.from_numpy(ref[k]).cuda() for k in "xys"), dense_t=(tA, tb, tc, tP),
             tA_bm=torch.from_numpy(tA_eval).cuda().t().contiguous(), tq=torch.from_numpy(tq_eval).cuda(), tP_bm=torch.from_numpy(K.p_tangent_values(tP, struct)).cuda())
    _CACHE[name] = r
    return r


def _jvp(r, tA_bm="given", tq="given", tP_bm="given"):
    eng = r["eng"]
    pick = lambda v, k: r[k] if isinstance(v, str) else v      # noqa: E731
    out = eng.jvp(r["A_bm"], *r["pt"], pick(tA_bm, "tA_bm"), pick(tq, "tq"), method="direct", P_bm=r["P_bm"], tP_bm=pick(tP_bm, "tP_bm"))
    assert eng.last_jvp_kernel == "ce_jvp_qp"
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out) + (eng.last_lsqr_iters.cpu().numpy(),)


@pytest.mark.parametrize("case", CASES)
def test_plan_and_dense_answer(case):
    r = _case(case)
    L = _lib.lib()
    assert r["eng"].qp_native and L.ce_qp_native(r["eng"]._h) == 1 and L.ce_adjoint_ns_variant(r["eng"]._h) == -1
    row = L.ce_qp_ns_variant(r["eng"]._h)
    assert row >= 0 and row == EXPECTED_ROW.get(case, row), row
    assert r["eng"].plan()["ns_variant"] == -1
    dx, dy, ds, st, its = _jvp(r)
    assert (its == 0).all() and ((st & ~4) == 0).all(), (st, its)
    tA, tb, tc, tP = r["dense_t"]
    want = K.dense_jvp(r["A"], r["Pm"], r["ref"]["x"], r["ref"]["y"], r["ref"]["s"], tA, tb, tc, tP, r["cones"])
    sel = (st == 0) & want[3] & (r["ref"]["status"] == 1)
    print(f"{case}: row {row}, status counts {np.bincount(st)}, compared {sel.mean():.3f}")
    assert sel.mean() >= 0.8, sel.mean()
    if case == "inactive_box":
        assert (st == 0).all(), st
    if case == "box_qp":
        act = ((r["ref"]["y"] - r["ref"]["s"]) > 0).sum(axis=1)
        print("  active bounds per instance: min", act.min(), "max", act.max())
        assert act.max() > 24          # the multi-wave row elimination is on the path
    e = np.max([np.abs(g - w).max(axis=1) / (1 + np.abs(w).max(axis=1)) for g, w in zip((dx, dy, ds), want[:3])], axis=0)[sel]
    print(f"  relative error vs the dense solve: max {e.max():.3e} median {np.median(e):.3e}")
    assert e.max() < 1e-5 and np.median(e) < 1e-8, (e.max(), np.median(e))


@pytest.mark.parametrize("case", CASES)
def test_transpose_identity_against_the_pivoting_adjoint_and_the_oracle(case):
    from oracle import oracle
    r = _case(case)
    eng, ref, tpl = r["eng"], r["ref"], r["tpl"]
    x, y, s = r["pt"]
    rng = np.random.default_rng(7)
    xb, yb = rng.standard_normal(ref["x"].shape), rng.standard_normal(ref["y"].shape)
    dx, dy, ds, st, _ = _jvp(r)
    dA, dq, adj, dP = eng.vjp(r["A_bm"], x, y, s, torch.from_numpy(xb).cuda(), torch.from_numpy(yb).cuda(), P_bm=r["P_bm"])
    torch.cuda.synchronize()
    adj = adj.cpu().numpy()
    sel = (st == 0) & (adj == 0) & (ref["status"] == 1)
    assert sel.mean() >= 0.8, (np.bincount(st), np.bincount(adj))
    lhs = (xb * dx).sum(axis=1) + (yb * dy).sum(axis=1)
    rhs = ((dA.t() * r["tA_bm"]).sum(dim=1) + (dq * r["tq"]).sum(dim=0) + (dP * r["tP_bm"]).sum(dim=1)).cpu().numpy()
    tA, tb, tc, tP = r["dense_t"]
    g = oracle.adjoint_batch(r["A"], r["b"], r["c"], r["cones"], ref["x"], ref["y"], ref["s"], xb, yb, P=r["Pm"], mode="dense")
    rhs_o = (g["dA"] * tA).sum(axis=(1, 2)) + (g["db"] * tb).sum(axis=1) + (g["dc"] * tc).sum(axis=1) + (g["dP"] * tP).sum(axis=(1, 2))
    for what, rh in (("k_backward_rt", rhs), ("oracle", rhs_o)):
        e = np.abs(lhs - rh) / (1 + np.abs(lhs) + np.abs(rh))
        print(f"{case} vs {what}: max |lhs - rhs| / (1 + |lhs| + |rhs|) = {e[sel].max():.3e}")
        assert (e[sel] < 1e-6).all(), (what, e[sel].max())
    assert np.abs(lhs[sel]).max() > 1e-3


@pytest.mark.parametrize("which", ["all", "P_alone"])
def test_qp_jvp_is_the_derivative_of_the_gpu_solution_map(which):
    """central differences of eng.solve (eps as test_direct_jvp_is_the_derivative_of_the_gpu_solution_map, h = 1e-5, bound 2e-4 (1 + max |jvp|)); a tangent in P
    alone, so that a dropped tP x term cannot hide behind the others"""
    from cvxpylayers_amd.interfaces.mi355_if import make_settings
    n, cones, B, seed = K.SHAPES["small_mixed"]
    B = 8
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=seed)
    Pm = K.quad_matrices(n, B, seed)
    struct = _upper_structure(n)
    eng = K.qp_engine(tpl, struct)
    st = make_settings(dict(acceleration_lookback=0, eps=1e-11, max_iters=200000))

    def solve(A_, b_, c_, P_):
        A_bm, q_t, P_bm = K.device_values(tpl, A_, b_, c_, P_, struct)
        x, y, s, _, status, _ = eng.solve(A_bm, q_t, st, P_bm=P_bm)
        assert (status.cpu().numpy() == 1).all()
        return A_bm, P_bm, (x, y, s)
    A_bm, P_bm, (x, y, s) = solve(A, b, c, Pm)
    rng = np.random.default_rng(3)
    tP = K.sym_tangent(B, n, 4)
    zero = which == "P_alone"
    tA, tb, tc = (np.zeros(t.shape) if zero else rng.standard_normal(t.shape) for t in (A, b, c))
    tA_eval, tq_eval = tpl.values_from_dense(tA, tb, tc)
    got = eng.jvp(A_bm, x, y, s, None if zero else torch.from_numpy(tA_eval).cuda().t().contiguous(), None if zero else torch.from_numpy(tq_eval).cuda(),
                  method="direct", P_bm=P_bm, tP_bm=torch.from_numpy(K.p_tangent_values(tP, struct)).cuda())
    assert eng.last_jvp_kernel == "ce_jvp_qp" and (got[3].cpu().numpy() == 0).all(), got[3]
    h = 1e-5
    plus = solve(A + h * tA, b + h * tb, c + h * tc, Pm + h * tP)[2]; minus = solve(A - h * tA, b - h * tb, c - h * tc, Pm - h * tP)[2]
    for name, g, p_, m_ in zip("xys", got[:3], plus, minus):
        fd = ((p_ - m_) / (2 * h)).cpu().numpy(); an = g.cpu().numpy()
        print(f"{which} d{name}: max |jvp - fd| = {np.abs(fd - an).max():.3e}, max |jvp| = {np.abs(an).max():.3e}")
        assert np.abs(fd - an).max() < 2e-4 * (1 + np.abs(an).max()), (name, np.abs(fd - an).max())
        assert np.abs(an).max() > 1e-3


def test_null_tangents():
    r = _case("small_mixed")
    dx, dy, ds, st, its = _jvp(r, None, None, None)
    assert (dx == 0).all() and (dy == 0).all() and (ds == 0).all() and (st == 0).all() and (its == 0).all()
    full = _jvp(r)
    zA, zq, zP = torch.zeros_like(r["tA_bm"]), torch.zeros_like(r["tq"]), torch.zeros_like(r["tP_bm"])
    for null, zeros in (((None, "given", "given"), (zA, "given", "given")), (("given", None, "given"), ("given", zq, "given")), (("given", "given", None), ("given", "given", zP))):
        a, b = _jvp(r, *null), _jvp(r, *zeros)
        assert (a[3] == 0).all() and (b[3] == 0).all()
        for u, v, f in zip(a[:3], b[:3], full[:3]):
            assert np.allclose(u, v, rtol=1e-9, atol=1e-12)          # a NULL tangent is a zero tangent
        assert np.abs(a[0] - full[0]).max() > 1e-6          # ... and each of the three tangents reaches the answer


def _assert_flagged(st, its, outs, who):
    assert (st[who] == 4).all() and (its == 0).all(), (st, its)
    assert all(np.isfinite(o).all() for o in outs)


def test_duplicated_equality_rows_are_flagged_and_keep_the_elimination_answer():
    """the mutation of test_gpu_jvp_direct.py on the small mixed shape (its two zero-cone rows: row 1 repeats row 0 in every second instance): status 4 and never
    4 | 8, no iterations, finite numbers; the other instances are solved as ever"""
    from oracle import oracle
    n, cones, A, b, c, Pm = K.instance("small_mixed")
    deg = np.arange(A.shape[0]) % 2 == 0
    A[deg, 1, :] = A[deg, 0, :]; b[deg, 1] = b[deg, 0]
    tpl = P.dense_template(n, cones); struct = _upper_structure(n)
    ref = oracle.solve_batch(A, b, c, cones, P=Pm, eps=1e-10, max_iters=200000)
    assert (ref["status"] == 1).mean() >= 0.9
    eng = K.qp_engine(tpl, struct)
    A_bm, q_t, P_bm = K.device_values(tpl, A, b, c, Pm, struct)
    r0 = _case("small_mixed")
    out = eng.jvp(A_bm, *(torch.from_numpy(ref[k]).cuda() for k in "xys"), r0["tA_bm"], r0["tq"], method="direct", P_bm=P_bm, tP_bm=r0["tP_bm"])
    torch.cuda.synchronize()
    st, its = out[3].cpu().numpy(), eng.last_lsqr_iters.cpu().numpy()
    _assert_flagged(st, its, [t.cpu().numpy() for t in out[:3]], deg)
    assert (st[~deg] == 0).all(), st


def test_a_solution_set_that_is_not_a_point_is_flagged():
    """P of rank n / 2 with c = P w and four nonnegative rows that are inactive at -w (n = 12, B = 24): default_rng(21) draws G (B, 12, 6), w (B, 12), A (B, 4, 12) in
    that order, P = G G^T / 12, b = -A w + 1.  The minimisers are (-w + null P) within the feasible set, Z^T (H + P) Z is singular.  The oracle solves 100 % of the
    batch at eps = 1e-10 and at 1e-4 with no active row."""
    from oracle import oracle
    B, n = 24, 12
    rng = np.random.default_rng(21)
    G = rng.standard_normal((B, n, n // 2)); Pm = G @ G.transpose(0, 2, 1) / n
    w = rng.standard_normal((B, n)); c = np.einsum("bij,bj->bi", Pm, w)
    A = rng.standard_normal((B, 4, n)); b = -np.einsum("bij,bj->bi", A, w) + 1.0
    cones = {"z": 0, "l": 4, "q": []}
    ref = oracle.solve_batch(A, b, c, cones, P=Pm, eps=1e-10, max_iters=200000)
    assert (ref["status"] == 1).mean() >= 0.9
    tpl = P.dense_template(n, cones); struct = _upper_structure(n)
    eng = K.qp_engine(tpl, struct)
    A_bm, q_t, P_bm = K.device_values(tpl, A, b, c, Pm, struct)
    tA_eval, tq_eval = tpl.values_from_dense(rng.standard_normal(A.shape), rng.standard_normal(b.shape), rng.standard_normal(c.shape))
    out = eng.jvp(A_bm, *(torch.from_numpy(ref[k]).cuda() for k in "xys"), torch.from_numpy(tA_eval).cuda().t().contiguous(), torch.from_numpy(tq_eval).cuda(),
                  method="direct", P_bm=P_bm, tP_bm=torch.from_numpy(K.p_tangent_values(K.sym_tangent(B, n, 2), struct)).cuda())
    torch.cuda.synchronize()
    _assert_flagged(out[3].cpu().numpy(), eng.last_lsqr_iters.cpu().numpy(), [t.cpu().numpy() for t in out[:3]], np.ones(B, bool))


def _plugin_inputs(struct_kind, B=6):
    """the equality QP (n = 6, p = 2) of test_quad_objective.py at the plugin boundary, with tangents; one infeasible instance is added by the caller"""
    from test_quad_objective import _eq_qp
    n, p = 6, 2
    Pm, q, F, g = _eq_qp(n, p, B, seed=1)
    cones = {"z": p, "l": 0, "q": [], "s": []}
    tpl = P.dense_template(n, cones)
    struct = _upper_structure(n) if struct_kind == "one_triangle" else K.full_structure(n)
    rng = np.random.default_rng(8)
    tP = K.sym_tangent(B, n, 9); tF = rng.standard_normal(F.shape); tg = rng.standard_normal(g.shape); tq_ = rng.standard_normal(q.shape)
    A_eval, q_eval = tpl.values_from_dense(F, g, q)
    tA_eval, tq_eval = tpl.values_from_dense(tF, tg, tq_)
    dev = torch.device("cuda", 0)
    vals = [torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (_p_values(Pm, struct).T, q_eval, A_eval)]
    tans = [torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (_p_values(tP, struct).T, tq_eval, tA_eval)]
    return n, cones, tpl, struct, vals, tans


@pytest.mark.parametrize("struct_kind", ["one_triangle", "full"])
def test_forward_ad_through_the_plugin_with_a_native_quadratic_objective(struct_kind, monkeypatch):
    """torch.autograd.forward_ad through _CvxpyLayer.apply(P_eval, ...) with jvp_mode="direct": the native route (ce_jvp_qp) against the same problem in epigraph
    form (CE_QP_EPIGRAPH=1: cone form, the linear-objective kernel); dx to the identity test's tolerance.  The default jvp_mode still refuses."""
    from cvxpylayers_amd.interfaces.mi355_if import MI355_ctx, _CvxpyLayer
    n, cones, tpl, struct, vals, tans = _plugin_inputs(struct_kind)
    got = {}
    for form in ("native", "epigraph"):
        if form == "epigraph":
            monkeypatch.setenv("CE_QP_EPIGRAPH", "1")
        ctx = MI355_ctx(struct, tpl.problem_data_index, cones, options={"eps": 1e-10, "max_iters": 200000, "jvp_mode": "direct"})
        with fwAD.dual_level():
            duals = [fwAD.make_dual(v.clone(), t) for v, t in zip(vals, tans)]
            primal, dual, info, _ = _CvxpyLayer.apply(*duals, ctx, {}, True, None)
            got[form] = (fwAD.unpack_dual(primal).tangent.clone(), fwAD.unpack_dual(primal).primal.clone())
            eng = (ctx if form == "native" else ctx.augmented()).engine(torch.device("cuda", 0))
            assert info["jvp"]["path"] == "direct" and eng.last_jvp_kernel == ("ce_jvp_qp" if form == "native" else "ce_jvp")
            assert (info["jvp"]["status"].cpu().numpy() == 0).all() and (info["jvp"]["iters"].cpu().numpy() == 0).all()
            if form == "native":
                assert ctx._aug_ctx is None and eng.qp_native
                with pytest.raises(NotImplementedError, match="jvp_mode='direct'"):
                    _CvxpyLayer.apply(*duals, ctx, {"jvp_mode": "lsqr"}, True, None)
    (dn, xn), (de, xe) = got["native"], got["epigraph"]
    err = ((dn - de).abs().amax(dim=1) / (1 + dn.abs().amax(dim=1) + de.abs().amax(dim=1))).max().item()
    print(f"{struct_kind}: max |dx native - dx epigraph| / (1 + |.| + |.|) = {err:.3e}; max |dx| = {dn.abs().max().item():.3e}")
    assert err < 1e-6 and dn.abs().max() > 1e-3


def test_failed_instances_return_nan_tangents_on_the_native_route():
    from cvxpylayers_amd.interfaces.mi355_if import MI355_ctx, _CvxpyLayer
    n, cones, tpl, struct, vals, tans = _plugin_inputs("one_triangle")
    P_eval, q_eval, A_eval = (v.clone() for v in vals)
    # instance 0: P indefinite (the native kernels fail it: test_indefinite_P_fails_loudly_in_the_native_kernels)
    diag = torch.from_numpy(np.flatnonzero(struct[0] == np.repeat(np.arange(n), np.diff(struct[1])))).cuda()
    P_eval[:, 0] = 0.0; P_eval[diag, 0] = 1.0; P_eval[diag[1], 0] = -1.0
    ctx = MI355_ctx(struct, tpl.problem_data_index, cones, options={"eps": 1e-9, "max_iters": 200000, "jvp_mode": "direct", "raise_on_error": False})
    import warnings
    with warnings.catch_warnings(), fwAD.dual_level():
        warnings.simplefilter("ignore")
        primal, dual, info, _ = _CvxpyLayer.apply(*(fwAD.make_dual(v, t) for v, t in zip((P_eval, q_eval, A_eval), tans)), ctx, {}, True, None)
        tp, td = fwAD.unpack_dual(primal).tangent, fwAD.unpack_dual(dual).tangent
        st = info["status"].cpu().numpy()
        assert st[0] < 0 and (st[1:] == 1).all(), st
        assert torch.isnan(tp[0]).all() and torch.isnan(td[0]).all() and torch.isfinite(tp[1:]).all() and torch.isfinite(td[1:]).all()
        assert info["jvp"]["path"] == "direct"


def test_frontend_layer_with_a_parametric_quad_form_under_forward_ad():
    """the template of test_quad_objective.py::test_frontend_layer_with_a_parametric_quad_form under fwAD with jvp_mode="direct", against forward-mode AD
    through the KKT solve (strictly positive optimum: the equality alone)"""
    from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery
    from cvxpylayers_amd.torch.templates import template_from_affine_builder
    n = 5

    def builder(Pp, qp):
        A = np.zeros((1 + n, n)); b = np.zeros(1 + n)
        A[0] = 1.0; b[0] = 1.0
        A[1:] = -np.eye(n)
        return A, b, qp, 0.5 * (Pp + Pp.T)
    tpl = template_from_affine_builder(builder, [(n, n), (n,)], {"z": 1, "l": n, "q": [], "s": []}, [VariableRecovery(slice(0, n), None, (n,))])
    layer = CvxpyLayer(template=tpl, solver_args={"eps": 1e-10, "max_iters": 200000, "jvp_mode": "direct"})
    torch.manual_seed(3)
    G = torch.randn(4, n, n, dtype=torch.float64, device="cuda")
    Pt = G @ G.transpose(1, 2) / n + torch.eye(n, dtype=torch.float64, device="cuda")
    qt = 0.1 * torch.randn(4, n, dtype=torch.float64, device="cuda")
    tPt = torch.randn(4, n, n, dtype=torch.float64, device="cuda"); tqt = torch.randn(4, n, dtype=torch.float64, device="cuda")
    with fwAD.dual_level():
        Pd, qd = fwAD.make_dual(Pt.clone(), tPt), fwAD.make_dual(qt.clone(), tqt)
        (x,) = layer(Pd, qd)
        xt = fwAD.unpack_dual(x).tangent
        assert layer.info["jvp"]["path"] == "direct" and (layer.info["jvp"]["status"].cpu().numpy() == 0).all()
        assert bool((fwAD.unpack_dual(x).primal > 1e-3).all())
        Ps = 0.5 * (Pd + Pd.transpose(1, 2))
        ones = torch.ones(4, 1, n, dtype=torch.float64, device="cuda")
        Kk = torch.cat([torch.cat([Ps, ones.transpose(1, 2)], dim=2), torch.cat([ones, torch.zeros(4, 1, 1, dtype=torch.float64, device="cuda")], dim=2)], dim=1)
        sol = torch.linalg.solve(Kk, torch.cat([-qd, torch.ones(4, 1, dtype=torch.float64, device="cuda")], dim=1)[:, :, None])[:, :, 0]
        want = fwAD.unpack_dual(sol).tangent[:, :n]
        print("frontend: max |jvp - KKT tangent| =", (xt - want).abs().max().item(), "max |tangent| =", want.abs().max().item())
        assert xt is not None and torch.allclose(xt, want, atol=1e-5), (xt - want).abs().max()


def test_refusals_that_stay_and_the_new_ones():
    """ce_jvp / ce_refine keep refusing a QP handle (-2); ce_jvp_qp / ce_refine_qp refuse a linear-objective handle and a PSD handle (-2)"""
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    r = _case("small_mixed")
    eng, B = r["eng"], r["A_bm"].shape[0]

    def buffers(e, B_):
        z = torch.zeros((B_, max(e.n, e.m, e.nnz_aug, e.nnz_p, 2)), dtype=torch.float64, device="cuda")
        return z, torch.zeros((B_,), dtype=torch.int32, device="cuda"), torch.zeros((e.n + 1, B_), dtype=torch.float64, device="cuda")
    z, zi, q0 = buffers(eng, B)
    rc = L.ce_jvp(eng._h, B, r["A_bm"].data_ptr(), eng.nnz_aug, None, 0, 0, z.data_ptr(), z.data_ptr(), z.data_ptr(), None, 0, None, 0, 0,
                  z.data_ptr(), z.data_ptr(), None, zi.data_ptr(), None, 1e-8, 1e-8, 1e8, 0, st)
    assert rc == -2 and b"epigraph" in L.ce_last_error()
    rc = L.ce_refine(eng._h, B, r["A_bm"].data_ptr(), eng.nnz_aug, q0.data_ptr(), q0.stride(0), q0.stride(1), z.data_ptr(), z.data_ptr(), z.data_ptr(), None, 1,
                     zi.data_ptr(), zi.data_ptr(), z.data_ptr(), st)
    assert rc == -2 and b"epigraph" in L.ce_last_error()
    for tpl in (P.dense_template(12, {"z": 2, "l": 6, "q": [4, 5]}), P.dense_template(4, {"z": 1, "s": [3]})):
        e = _engine(tpl)
        assert L.ce_qp_native(e._h) == 0 and L.ce_qp_ns_variant(e._h) == -1
        z, zi, q0 = buffers(e, 3)
        rc = L.ce_jvp_qp(e._h, 3, z.data_ptr(), e.nnz_aug, z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None, 0, None, 0, 0, None,
                         z.data_ptr(), z.data_ptr(), None, zi.data_ptr(), None, st)
        assert rc == -2 and b"ce_qp_native" in L.ce_last_error(), (rc, L.ce_last_error())
        rc = L.ce_refine_qp(e._h, 3, z.data_ptr(), e.nnz_aug, q0.data_ptr(), q0.stride(0), q0.stride(1), z.data_ptr(), z.data_ptr(), z.data_ptr(), z.data_ptr(), None, 1,
                            zi.data_ptr(), zi.data_ptr(), z.data_ptr(), st)
        assert rc == -2 and b"ce_qp_native" in L.ce_last_error(), (rc, L.ce_last_error())
    torch.cuda.synchronize()
    with pytest.raises(NotImplementedError, match="method='direct'"):
        eng.jvp(r["A_bm"], *r["pt"], r["tA_bm"], r["tq"], P_bm=r["P_bm"], tP_bm=r["tP_bm"])

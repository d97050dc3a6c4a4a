"""The optimal value as a layer output with envelope-theorem gradients: k_value / k_value_vjp_rows / k_value_vjp_tile behind ce_value, ce_value_jvp, ce_value_vjp,
interfaces/optimal_value.py and CvxpyLayer.forward(return_value=True).  The numpy statements of the formulas, the shapes and the bounds are in value_kit.py:
  * scalars: |got - want| <= 4 L 2^-53 sum |terms| for a sum of L terms; gradient entries: within 4 ulp of the exact product (both derived, not measured);
  * layer against the oracle: the project's forward parity bound on a linear functional of x, 1e-6 (1 + sum |c_j x_j|);
  * gradients against the existing route (c^T x + d built in torch, backward through the adjoint): 1e-6 (1 + max |want|) on instances whose adjoint status is 0.
Every case fails on a library without the three entry points and on a frontend without the keyword."""
import dataclasses
import functools

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import ref_cases
import value_kit as vk
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = 777.25
GUARD = 37
LAYOUTS = [("major", "major"), ("minor", "minor"), ("major", "minor"), ("minor", "major")]


def _engine(tpl, struct=None):
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
    return ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, DEV, p_structure=struct[:2] if struct is not None else None)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _point(name):
    """a kernel shape at the oracle's point (computed once, shared, never changed): template, engine, boundary values with a non-zero constant d, (x, y)"""
    from oracle import oracle
    n, cones, B, seed, sparse = vk.KERNEL_SHAPES[name]
    if sparse:
        A, b, c, pattern, b_pattern = vk.sparse_instance(n, cones, B, seed)
        tpl = P.dense_template(n, cones, pattern=pattern, b_pattern=b_pattern)
        assert (np.diff(tpl.indptr)[:n] == 0).sum() == 1 and tpl.indptr[n + 1] - tpl.indptr[n] < tpl.m
    else:
        A, b, c = P.generate(n, cones, B, seed=seed)
        tpl = P.dense_template(n, cones)
    ref = oracle.solve_batch(A, b, c, cones, eps=1e-10, max_iters=400000)
    assert (ref["status"] == 1).all(), ref["status"]
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    q_eval[n] = np.random.default_rng(seed + 7).standard_normal(B)
    return dict(tpl=tpl, eng=_engine(tpl), A_eval=A_eval, q_eval=q_eval, x=ref["x"], y=ref["y"], B=B, A=A, b=b, c=c, cones=cones)


def _struct_dev(struct):
    pr, pc, _ = vk.p_entries(struct)
    return _cuda(pr.astype(np.int32)), _cuda(pc.astype(np.int32))


def _raw_vjp(eng, x, y, g, skip=None, A_layout="major", q_layout="minor", struct=None, want=(True, True)):
    """ce_value_vjp through the C ABI into buffers with guard bands: returns numpy dA (nnz_aug, B), dq (n+1, B), dP (B, nnz_p); the bands must come back untouched"""
    B, K, n = x.shape[0], eng.nnz_aug, eng.n
    nnz_p = len(struct[0]) if struct is not None else 0

    def guarded(size):
        buf = torch.full((2 * GUARD + size,), SENTINEL, dtype=torch.float64, device=DEV)
        return buf, buf[GUARD:GUARD + size]
    bA, vA = guarded(K * B); bq, vq = guarded((n + 1) * B); bP, vP = guarded(max(nnz_p * B, 1))
    sA = (1, K) if A_layout == "major" else (B, 1)
    sq = (1, n + 1) if q_layout == "major" else (B, 1)
    pst = _struct_dev(struct) if struct is not None else None
    sk = skip.view(torch.uint8) if skip is not None else None
    rc = _lib.lib().ce_value_vjp(eng._h, B, x.data_ptr(), y.data_ptr(), g.data_ptr(), sk.data_ptr() if sk is not None else None,
                                 vA.data_ptr() if want[0] else None, *sA, vq.data_ptr() if want[1] else None, *sq,
                                 vP.data_ptr() if nnz_p else None, pst[0].data_ptr() if pst else None, pst[1].data_ptr() if pst else None, nnz_p, eng._stream())
    _lib.check(rc, "ce_value_vjp")
    torch.cuda.synchronize()
    for buf, size, written in ((bA, K * B, want[0]), (bq, (n + 1) * B, want[1]), (bP, max(nnz_p * B, 1), nnz_p > 0)):
        assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + size:] == SENTINEL).all(), "a guard band was written"
        if not written:
            assert (buf == SENTINEL).all(), "an output that was not asked for was written"
    dA = (vA.view(B, K).t() if A_layout == "major" else vA.view(K, B)).cpu().numpy()
    dq = (vq.view(B, n + 1).t() if q_layout == "major" else vq.view(n + 1, B)).cpu().numpy()
    return dA, dq, (vP[:nnz_p * B].view(B, nnz_p).cpu().numpy() if nnz_p else None)


def _tangents(tpl, B, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((tpl.nnz_aug, B)), rng.standard_normal((tpl.n + 1, B))


# ------------------------------------------------------------------------------------------------ 1. kernels against numpy on the same point
@pytest.mark.parametrize("name", list(vk.KERNEL_SHAPES))
def test_kernels_equal_the_numpy_formulas_at_the_oracles_point(name):
    r = _point(name)
    tpl, eng, B = r["tpl"], r["eng"], r["B"]
    x, y = _cuda(r["x"]), _cuda(r["y"])
    want = vk.objective(tpl, r["A_eval"], r["q_eval"], r["x"], r["y"])
    # ce_value: the reference's (., B) contiguous arrays and batch-minor views of batch-major storage, read without a copy
    for how in ("minor", "major_view"):
        A_t, q_t = _cuda(r["A_eval"]), _cuda(r["q_eval"])
        if how == "major_view":
            A_t, q_t = A_t.t().contiguous().t(), q_t.t().contiguous().t()
        pobj, dobj = eng.value(A_t, q_t, x, y)
        vk.assert_scalar(pobj.cpu().numpy(), want["pobj"], want["pobj_abs"], want["pobj_terms"], f"pobj ({how})")
        vk.assert_scalar(dobj.cpu().numpy(), want["dobj"], want["dobj_abs"], want["dobj_terms"], f"dobj ({how})")
    # ce_value_jvp: every tangent, each one alone, none
    tA, tq = _tangents(tpl, B, 11)
    tA_bm, tq_t = _cuda(tA.T), _cuda(tq)
    for use_A, use_q in ((True, True), (True, False), (False, True)):
        got = eng.value_jvp(x, y, tA_bm if use_A else None, tq_t if use_q else None)
        an, scale, L = vk.value_jvp(tpl, r["x"], r["y"], tA if use_A else None, tq if use_q else None)
        vk.assert_scalar(got.cpu().numpy(), an, scale, L, f"tangent (A {use_A}, q {use_q})")
    assert (eng.value_jvp(x, y).cpu().numpy() == 0).all()
    got = eng.value_jvp(x, y, tA_bm, _cuda(tq.T).t())          # tq as a batch-minor view of batch-major storage
    an, scale, L = vk.value_jvp(tpl, r["x"], r["y"], tA, tq)
    vk.assert_scalar(got.cpu().numpy(), an, scale, L, "tangent (tq batch-major storage)")
    # ce_value_vjp: both stride conventions of dA and of dq, guard bands around the outputs
    g = np.random.default_rng(5).standard_normal(B)
    w_dA, w_dq, _ = vk.value_vjp(tpl, r["x"], r["y"], g)
    for A_layout, q_layout in LAYOUTS:
        dA, dq, _ = _raw_vjp(eng, x, y, _cuda(g), A_layout=A_layout, q_layout=q_layout)
        vk.assert_ulp(dA, w_dA, f"dA {A_layout}")
        vk.assert_ulp(dq, w_dq, f"dq {q_layout}")
    # outputs that are not wanted are not written
    for want_out in ((True, False), (False, True)):
        for A_layout in ("major", "minor"):
            dA, dq, _ = _raw_vjp(eng, x, y, _cuda(g), A_layout=A_layout, q_layout="minor", want=want_out)
            if want_out[0]:
                vk.assert_ulp(dA, w_dA, "dA alone")
            else:
                vk.assert_ulp(dq, w_dq, "dq alone")


@pytest.mark.parametrize("kind", ["full", "one_triangle"])
def test_kernels_with_a_quadratic_objective(kind):
    """n = 6, {z: 2, l: 4}: P in a structure with both triangles and in one triangle (an off-diagonal entry counts twice), on a handle that knows the structure
    and on one that does not (the structure is an argument of the calls)"""
    from oracle import oracle
    from qp_ns_kit import full_structure, quad_matrices
    from test_quad_objective import _p_values, _upper_structure
    n, cones, B, seed = vk.QP_SHAPE
    struct = full_structure(n) if kind == "full" else _upper_structure(n)
    assert vk.one_triangle(*vk.p_entries(struct)[:2]) == (kind == "one_triangle")
    A, b, c = P.generate(n, cones, B, seed=seed)
    Pm = quad_matrices(n, B, seed)
    ref = oracle.solve_batch(A, b, c, cones, P=Pm, eps=1e-10, max_iters=400000)
    assert (ref["status"] == 1).all()
    tpl = P.dense_template(n, cones)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    q_eval[n] = 0.75
    P_vals = np.ascontiguousarray(_p_values(Pm, struct))
    rng = np.random.default_rng(9)
    tP = rng.standard_normal((B, n, n)); tP_vals = np.ascontiguousarray(_p_values(tP + tP.transpose(0, 2, 1), struct))
    tA, tq = _tangents(tpl, B, 12)
    g = rng.standard_normal(B)
    x, y, pst = _cuda(ref["x"]), _cuda(ref["y"]), _struct_dev(struct)
    want = vk.objective(tpl, A_eval, q_eval, ref["x"], ref["y"], P_vals, struct)
    gap = np.abs(want["pobj"] - want["dobj"]).astype(float)
    assert (gap < 1e-7 * (1 + np.abs(want["pobj"]).astype(float))).all(), gap          # (the formulas themselves: primal = dual at the oracle's point)
    an, scale, L = vk.value_jvp(tpl, ref["x"], ref["y"], tA, tq, tP_vals, struct)
    an_P, scale_P, L_P = vk.value_jvp(tpl, ref["x"], ref["y"], None, None, tP_vals, struct)
    w_dA, w_dq, w_dP = vk.value_vjp(tpl, ref["x"], ref["y"], g, struct)
    for eng in (_engine(tpl), _engine(tpl, struct)):
        pobj, dobj = eng.value(_cuda(A_eval), _cuda(q_eval), x, y, P_bm=_cuda(P_vals), p_structure=pst)
        vk.assert_scalar(pobj.cpu().numpy(), want["pobj"], want["pobj_abs"], want["pobj_terms"], "pobj")
        vk.assert_scalar(dobj.cpu().numpy(), want["dobj"], want["dobj_abs"], want["dobj_terms"], "dobj")
        got = eng.value_jvp(x, y, _cuda(tA.T), _cuda(tq), _cuda(tP_vals), pst)
        vk.assert_scalar(got.cpu().numpy(), an, scale, L, "tangent")
        got = eng.value_jvp(x, y, None, None, _cuda(tP_vals), pst)
        vk.assert_scalar(got.cpu().numpy(), an_P, scale_P, L_P, "tangent of P alone")
        for A_layout, q_layout in LAYOUTS[:2]:
            dA, dq, dP = _raw_vjp(eng, x, y, _cuda(g), A_layout=A_layout, q_layout=q_layout, struct=struct)
            vk.assert_ulp(dA, w_dA, "dA"); vk.assert_ulp(dq, w_dq, "dq"); vk.assert_ulp(dP, w_dP, "dP")
        # the row mask reaches dP too
        skip = torch.zeros(B, dtype=torch.bool, device=DEV); skip[1] = True
        xn = x.clone(); xn[1] = float("nan")
        dA, dq, dP = _raw_vjp(eng, xn, y, _cuda(g), skip=skip, struct=struct)
        assert (dP[1] == 0).all() and (dA[:, 1] == 0).all() and (dq[:, 1] == 0).all()
        keep = np.arange(B) != 1
        vk.assert_ulp(dP[keep], w_dP[keep], "dP of the other rows")


def test_tile_kernel_gathers_from_global_memory_when_a_tile_exceeds_lds():
    """the batch-minor layout stages 64 instances' x and y in LDS; n + m = 350 does not fit (65 * 350 * 8 bytes > 160 KiB), so the lanes gather instead: the other
    path of k_value_vjp_tile.  The formulas hold at any point: x, y are random here (no solve of a 200-variable program is needed to check products)."""
    n, cones, B = 200, {"z": 0, "l": 150, "q": []}, 65
    rng = np.random.default_rng(3)
    pattern = rng.random((150, n)) < 0.05
    tpl = P.dense_template(n, cones, pattern=pattern)
    assert 65 * (n + tpl.m) * 8 > 160 * 1024
    eng = _engine(tpl)
    xn, yn, g = rng.standard_normal((B, n)), rng.standard_normal((B, tpl.m)), rng.standard_normal(B)
    w_dA, w_dq, _ = vk.value_vjp(tpl, xn, yn, g)
    skip = torch.zeros(B, dtype=torch.bool, device=DEV); skip[[2, 64]] = True
    xs = _cuda(xn); xs[2] = float("nan")
    for A_layout, q_layout in LAYOUTS[:2]:
        dA, dq, _ = _raw_vjp(eng, _cuda(xn), _cuda(yn), _cuda(g), A_layout=A_layout, q_layout=q_layout)
        vk.assert_ulp(dA, w_dA, f"dA {A_layout}"); vk.assert_ulp(dq, w_dq, f"dq {q_layout}")
        dA_s, dq_s, _ = _raw_vjp(eng, xs, _cuda(yn), _cuda(g), skip=skip, A_layout=A_layout, q_layout=q_layout)
        keep = ~skip.cpu().numpy()
        assert (dA_s[:, ~keep] == 0).all() and (dq_s[:, ~keep] == 0).all()
        assert np.array_equal(dA_s[:, keep], dA[:, keep]) and np.array_equal(dq_s[:, keep], dq[:, keep])


# ------------------------------------------------------------------------------------------------ 2. batch purity
def test_an_instances_scalars_do_not_depend_on_the_batch():
    r = _point("dense_b65")
    tpl, eng, B = r["tpl"], r["eng"], r["B"]
    tA, tq = _tangents(tpl, B, 13)
    A_bm, q_bm, x, y, tA_bm, tq_bm = (_cuda(a) for a in (r["A_eval"].T, r["q_eval"].T, r["x"], r["y"], tA.T, tq.T))

    def run(idx):
        idx = torch.as_tensor(idx, device=DEV)
        sel = lambda t: t.index_select(0, idx).contiguous()
        pobj, dobj = eng.value(sel(A_bm).t(), sel(q_bm).t(), sel(x), sel(y))
        return pobj, dobj, eng.value_jvp(sel(x), sel(y), sel(tA_bm), sel(tq_bm).t())
    whole = run(list(range(B)))
    for i in (0, 3, 63, 64):
        alone = run([i])
        moved = run([7, 1, 64, 2, 0, i, 5])          # the same instance at position 5 of a batch of 7
        for w, a, m_ in zip(whole, alone, moved):
            assert torch.equal(w[i:i + 1], a) and torch.equal(w[i:i + 1], m_[5:6]), (i, w[i], a, m_[5])


# ------------------------------------------------------------------------------------------------ 3. the skip mask
@pytest.mark.parametrize("A_layout,q_layout", LAYOUTS[:2])
def test_masked_rows_are_exact_zeros_and_the_others_unchanged(A_layout, q_layout):
    r = _point("dense_b65")
    eng, B = r["eng"], r["B"]
    g = _cuda(np.random.default_rng(6).standard_normal(B))
    x, y = _cuda(r["x"]), _cuda(r["y"])
    clean = _raw_vjp(eng, x, y, g, A_layout=A_layout, q_layout=q_layout)
    skip = torch.zeros(B, dtype=torch.bool, device=DEV); skip[::3] = True; skip[64] = True
    xn, yn, gn = x.clone(), y.clone(), g.clone()
    xn[skip] = float("nan"); yn[skip] = float("nan"); gn[skip] = float("nan")
    masked = _raw_vjp(eng, xn, yn, gn, skip=skip, A_layout=A_layout, q_layout=q_layout)
    sk = skip.cpu().numpy()
    for c_, m_ in zip(clean[:2], masked[:2]):
        assert (m_[:, sk] == 0).all() and not np.isnan(m_).any()
        assert np.array_equal(m_[:, ~sk], c_[:, ~sk])
    # a mask of zeros is no mask
    same = _raw_vjp(eng, x, y, g, skip=torch.zeros(B, dtype=torch.bool, device=DEV), A_layout=A_layout, q_layout=q_layout)
    assert np.array_equal(same[0], clean[0]) and np.array_equal(same[1], clean[1])


# ------------------------------------------------------------------------------------------------ 4. layer against the oracle
def _full(template, **kw):
    """the same template returning the whole primal and the whole dual vector"""
    from cvxpylayers_amd.torch import VariableRecovery
    n, m = int(template.q_map.shape[0]) - 1, int(template.A_structure[2][0])
    return dataclasses.replace(template, var_recover=[VariableRecovery(slice(0, n), None, (n,)), VariableRecovery(None, slice(0, m), (m,), source="dual")], **kw)


def _cone_template(template):
    idx, ptr, (m, np1) = template.A_structure
    return P.ConeTemplate(n=np1 - 1, m=m, indices=np.asarray(idx), indptr=np.asarray(ptr), cones=dict(template.cone_dims))


def _dense_P(template, P_eval):
    """(B, n, n) symmetric matrices of P_eval (nnz_p, B) in the template's structure"""
    pr, pc, _ = vk.p_entries(template.P_structure)
    n = template.P_structure[2][0]
    Pd = np.zeros((P_eval.shape[1], n, n))
    Pd[:, pr, pc] = P_eval.T
    if vk.one_triangle(pr, pc):
        Pd = Pd + Pd.transpose(0, 2, 1) - Pd * np.eye(n)
    return Pd


def _check_layer_value(template, params, batched, solver_args=None, expect_path=None):
    """value of return_value=True against the oracle's, info["objective"] against the kit's formulas on the returned point"""
    from oracle import oracle
    from cvxpylayers_amd.torch import CvxpyLayer
    template = _full(template)
    layer = CvxpyLayer(template=template, solver_args={**ref_cases.SOLVER_ARGS, **(solver_args or {})})
    out = layer(*[_cuda(p) for p in params], return_value=True)
    assert len(out) == 3
    xr, yr, val = out
    A_eval, q_eval, P_eval, _ = vk.canon_values(template, params)
    B = A_eval.shape[1]
    assert val.dtype == torch.float64 and tuple(val.shape) == ((B,) if batched else ())
    if expect_path is not None:
        assert layer.ctx.solver_ctx.engine(DEV).last_path == expect_path
    tplc = _cone_template(template)
    A, b, c = tplc.dense_from_values(A_eval, q_eval)
    Pd = _dense_P(template, P_eval) if P_eval is not None else None
    ref = oracle.solve_batch(A, b, c, tplc.cones, P=Pd, eps=1e-10, max_iters=400000)
    assert (ref["status"] == 1).all()
    want = np.einsum("bj,bj->b", c, ref["x"]) + q_eval[tplc.n] + (0.5 * np.einsum("bi,bij,bj->b", ref["x"], Pd, ref["x"]) if Pd is not None else 0.0)
    got = val.detach().cpu().numpy().reshape(-1)
    bound = 1e-6 * (1 + np.abs(c * ref["x"]).sum(axis=1))
    print("value:", got, "oracle:", want, "max error", np.abs(got - want).max(), "bound", bound.min())
    assert (np.abs(got - want) <= bound).all(), (got, want, bound)
    obj = layer.info["objective"]
    assert not obj["primal"].requires_grad and not obj["dual"].requires_grad and tuple(obj["primal"].shape) == tuple(val.shape) == tuple(obj["dual"].shape)
    xn, yn = xr.detach().cpu().numpy().reshape(B, -1), yr.detach().cpu().numpy().reshape(B, -1)
    k = vk.objective(tplc, A_eval, q_eval, xn, yn, P_eval.T if P_eval is not None else None, template.P_structure)
    vk.assert_scalar(obj["primal"].cpu().numpy().reshape(-1), k["pobj"], k["pobj_abs"], k["pobj_terms"], "info primal")
    vk.assert_scalar(obj["dual"].cpu().numpy().reshape(-1), k["dobj"], k["dobj_abs"], k["dobj_terms"], "info dual")
    assert torch.equal(val.detach(), obj["primal"])
    # without the keyword the outputs are what they were
    assert len(layer(*[_cuda(p) for p in params])) == 2
    return layer


def test_layer_value_ridge_unbatched_and_batch_of_one():
    cs = ref_cases.case_ridge_unbatched()
    _check_layer_value(cs["template"], cs["params"], batched=False)
    _check_layer_value(cs["template"], [p[None] for p in cs["params"]], batched=True)


def test_layer_value_sdp():
    cs = ref_cases.case_sdp_symmetric_primal_and_psd_dual()
    _check_layer_value(cs["template"], cs["params"], batched=True)


def test_layer_value_shared_a_portfolio(monkeypatch):
    from cvxpylayers_amd.torch import VariableRecovery
    from cvxpylayers_amd.torch.templates import template_from_affine_builder
    monkeypatch.setenv("CE_CONST_A", "1")
    A, b, c, cones, _ = P.portfolio_c5_batch(6, nw=60, kf=9)
    nw = 60
    tpl = template_from_affine_builder(lambda mu: (A, b, np.concatenate([-mu, [1.0]])), [(nw,)], cones, [VariableRecovery(slice(0, nw), None, (nw,))])
    _check_layer_value(tpl, [-c[:, :nw]], batched=True, expect_path="const_a")


def _qp_template():
    """test_quad_objective.py::test_frontend_layer_with_a_parametric_quad_form: min 1/2 x^T P x + q^T x  s.t.  1^T x = 1, x >= 0, P and q parameters"""
    from cvxpylayers_amd.torch import VariableRecovery
    from cvxpylayers_amd.torch.templates import template_from_affine_builder
    n = 5

    def builder(Pp, qp):
        A = np.zeros((1 + n, n)); b = np.zeros(1 + n)
        A[0] = 1.0; b[0] = 1.0
        A[1:] = -np.eye(n)
        return A, b, qp, 0.5 * (Pp + Pp.T)
    tpl = template_from_affine_builder(builder, [(n, n), (n,)], {"z": 1, "l": n, "q": [], "s": []}, [VariableRecovery(slice(0, n), None, (n,))])
    rng = np.random.default_rng(2)
    G = rng.standard_normal((4, n, n))
    return tpl, [G @ G.transpose(0, 2, 1) / n + 0.5 * np.eye(n), 0.3 * rng.standard_normal((4, n))]


@pytest.mark.parametrize("form", ["native", "epigraph"])
def test_layer_value_and_gradients_with_a_quadratic_objective(form, monkeypatch):
    if form == "epigraph":
        monkeypatch.setenv("CE_QP_EPIGRAPH", "1")
    tpl, params = _qp_template()
    layer = _check_layer_value(tpl, params, batched=True)
    eng = layer.ctx.solver_ctx.engine(DEV)
    assert eng.qp_native and (form == "native") == (layer.ctx.solver_ctx._aug_ctx is None)
    # gradients of the value against the kit's envelope formulas pushed through the template's maps
    Pt, qt = (_cuda(p).requires_grad_() for p in params)
    xr, yr, val = layer(Pt, qt, return_value=True)
    w = _cuda(np.random.default_rng(3).standard_normal(val.shape[0]))
    gP, gq = torch.autograd.grad((w * val).sum(), [Pt, qt])
    assert layer.info["adjoint"]["status"] is None
    dA, dq, dP = vk.value_vjp(_cone_template(layer.template), xr.detach().cpu().numpy(), yr.detach().cpu().numpy(), w.cpu().numpy(), layer.template.P_structure)
    wP, wq = vk.param_grads(layer.template, dA, dq, dP.T)
    for got, want in ((gP, wP), (gq, wq)):
        err = np.abs(got.cpu().numpy() - want).max()
        print("max error", err, "of", np.abs(want).max())
        assert err <= 1e-6 * (1 + np.abs(want).max())
    assert np.abs(wP).max() > 1e-3 and np.abs(wq).max() > 1e-3


# ------------------------------------------------------------------------------------------------ 5. gradients two ways
N12, CONES12 = 12, {"z": 2, "l": 6, "q": [4, 5]}


@functools.lru_cache(maxsize=None)
def _layer12(with_d=True):
    from cvxpylayers_amd.torch import CvxpyLayer
    return CvxpyLayer(template=vk.identity_template(N12, CONES12, with_d=with_d), solver_args=ref_cases.SOLVER_ARGS)


def _params12(B, seed, requires_grad=True):
    A, b, c = P.generate(N12, CONES12, B, seed=seed)
    d = np.random.default_rng(seed + 3).standard_normal(B)
    return [(_cuda(p).requires_grad_() if requires_grad else _cuda(p)) for p in (A, b, c, d)]


def test_gradients_of_the_value_two_ways():
    layer, B = _layer12(), 16
    tplc = _cone_template(layer.template)
    w = _cuda(np.random.default_rng(8).standard_normal(B))
    params = _params12(B, 21)
    x, y, val = layer(*params, return_value=True)
    g_val = torch.autograd.grad((w * val).sum(), params)
    assert layer.info["adjoint"]["status"] is None
    # (a) the kit's envelope formulas at the returned point, pushed through the template's maps in numpy
    dA, dq, _ = vk.value_vjp(tplc, x.detach().cpu().numpy(), y.detach().cpu().numpy(), w.cpu().numpy())
    for name, got, want in zip("Abcd", g_val, vk.param_grads(layer.template, dA, dq)):
        err = np.abs(got.cpu().numpy() - want).max()
        print(f"(a) d/d{name}: max error {err:.3e} of {np.abs(want).max():.3e}")
        assert err <= 1e-6 * (1 + np.abs(want).max()), name
    assert (g_val[3] == w).all()
    # (b) the existing route: c^T x + d built in torch from the layer's variable, backward through the adjoint
    params2 = _params12(B, 21)
    x2, _ = layer(*params2)
    g_adj = torch.autograd.grad((w * ((params2[2] * x2).sum(dim=1) + params2[3])).sum(), params2)
    ok = (layer.info["adjoint"]["status"] == 0).cpu().numpy()
    print("adjoint status 0 on", ok.mean())
    assert ok.mean() >= 0.8
    for name, got, want in zip("Abcd", g_val, g_adj):
        got, want = got.cpu().numpy()[ok], want.cpu().numpy()[ok]
        err = np.abs(got - want).max()
        print(f"(b) d/d{name}: max error {err:.3e} of {np.abs(want).max():.3e}")
        assert err <= 1e-6 * (1 + np.abs(want).max()), name
    # a loss that uses a variable AND the value: both paths add into one parameter gradient
    params3 = _params12(B, 21)
    x3, y3, val3 = layer(*params3, return_value=True)
    wx = _cuda(np.random.default_rng(9).standard_normal((B, N12)))
    g_both = torch.autograd.grad((wx * x3).sum() + (w * val3).sum(), params3)
    assert (layer.info["adjoint"]["status"] is not None)
    params4 = _params12(B, 21)
    x4, _ = layer(*params4)
    g_x = torch.autograd.grad((wx * x4).sum(), params4)
    for name, both, a, b_ in zip("Abcd", g_both, g_x, g_val):
        assert torch.allclose(both, a + b_, rtol=1e-12, atol=1e-14), name


# ------------------------------------------------------------------------------------------------ 6. central differences of the GPU value
def test_value_tangent_is_the_derivative_of_the_gpu_value():
    """recipe and bound of test_gpu_jvp_direct.py::test_direct_jvp_is_the_derivative_of_the_gpu_solution_map: eps 1e-11, h = 1e-5, 2e-4 (1 + |an|)"""
    from cvxpylayers_amd.interfaces.mi355_if import make_settings
    n, cones, B = N12, CONES12, 8
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=7)
    eng = _engine(tpl)
    st = make_settings(dict(acceleration_lookback=0, eps=1e-11, max_iters=200000))
    rng = np.random.default_rng(3)
    dA, db, dc = rng.standard_normal(A.shape), rng.standard_normal(b.shape), rng.standard_normal(c.shape)

    def solve(A_, b_, c_):
        A_eval, q_eval = tpl.values_from_dense(A_, b_, c_)
        A_bm = _cuda(A_eval.T); q_t = _cuda(q_eval)
        x, y, s, _, status, _ = eng.solve(A_bm, q_t, st)
        assert (status.cpu().numpy() == 1).all()
        return eng.value(A_bm.t(), q_t, x, y)[0].cpu().numpy(), x, y
    _, x, y = solve(A, b, c)
    tA_eval, tq_eval = tpl.values_from_dense(dA, db, dc)
    an = eng.value_jvp(x, y, _cuda(tA_eval.T), _cuda(tq_eval)).cpu().numpy()
    h = 1e-5
    fd = (solve(A + h * dA, b + h * db, c + h * dc)[0] - solve(A - h * dA, b - h * db, c - h * dc)[0]) / (2 * h)
    print("max |tangent - fd| =", np.abs(fd - an).max(), "max |tangent| =", np.abs(an).max())
    assert (np.abs(fd - an) < 2e-4 * (1 + np.abs(an))).all(), (fd, an)


# ------------------------------------------------------------------------------------------------ 7. forward mode
def test_forward_mode_tangent_of_the_value():
    from cvxpylayers_amd.interfaces import optimal_value
    from cvxpylayers_amd.interfaces.mi355_if import MI355_ctx, _CvxpyLayer
    r = _point("dense_b5")
    tpl, B = r["tpl"], r["B"]
    ctx = MI355_ctx(None, tpl.problem_data_index, r["cones"], options=ref_cases.SOLVER_ARGS)
    tA, tq = _tangents(tpl, B, 14)
    for how in ("minor", "major_view"):
        A_t, q_t, tA_t, tq_t = (_cuda(a) for a in (r["A_eval"], r["q_eval"], tA, tq))
        if how == "major_view":
            A_t, q_t, tA_t, tq_t = (t.t().contiguous().t() for t in (A_t, q_t, tA_t, tq_t))
        primal, dual, info, _ = _CvxpyLayer.apply(None, q_t, A_t, ctx, {}, True, None)
        Ag, qg = A_t.clone().requires_grad_(), q_t.clone().requires_grad_()
        val = optimal_value(None, qg, Ag, primal, dual, ctx)
        gA, gq = torch.autograd.grad(val.sum(), [Ag, qg])
        assert gA.stride() == Ag.stride() and tuple(gA.shape) == tuple(Ag.shape)          # the gradient comes back in the storage order of the input
        want = ((gA.cpu().numpy().astype(vk.LD) * tA).sum(axis=0) + (gq.cpu().numpy().astype(vk.LD) * tq).sum(axis=0)).astype(float)
        with fwAD.dual_level():
            vd = optimal_value(None, fwAD.make_dual(q_t, tq_t), fwAD.make_dual(A_t, tA_t), primal, dual, ctx, info=info)
            tangent = fwAD.unpack_dual(vd).tangent
            assert tangent is not None and torch.equal(fwAD.unpack_dual(vd).primal, val.detach())
            got = tangent.cpu().numpy()
        print("forward mode vs <grad, tangent>:", np.abs(got - want).max())
        assert (np.abs(got - want) <= 1e-12 * (1 + np.abs(want))).all(), (got, want)
        assert "jvp" not in info and "objective" in info          # no system was solved for it
    # through the frontend: the tangents of the parameters reach the value through the maps
    layer = _layer12()
    params = _params12(B, 21, requires_grad=False)
    tangents = [_cuda(np.random.default_rng(30 + k).standard_normal(tuple(p.shape))) for k, p in enumerate(params)]
    with fwAD.dual_level():
        out = layer(*[fwAD.make_dual(p, t) for p, t in zip(params, tangents)], return_value=True)
        got = fwAD.unpack_dual(out[-1]).tangent.cpu().numpy()
    pg = [p.clone().requires_grad_() for p in params]
    val = layer(*pg, return_value=True)[-1]
    want = np.zeros(B)
    for i in range(B):
        gi = torch.autograd.grad(val[i], pg, retain_graph=True)
        want[i] = sum(float((g_[i].double() * t[i]).sum()) for g_, t in zip(gi, tangents))
    assert (np.abs(got - want) <= 1e-12 * (1 + np.abs(want))).all(), (got, want)


# ------------------------------------------------------------------------------------------------ 8. no system is solved
def _duplicated_rows_batch(B=24, seed=11):
    """the construction of test_gpu_tri_jvp.py::test_duplicated_equality_rows_are_flagged_and_resolved: every second instance has a redundant equality row;
    as there, the instances the oracle does not solve are left out (at least 80 % stay)"""
    from oracle import oracle
    n, cones = 12, {"z": 4, "l": 8, "q": [5]}
    A, b, c = P.generate(n, cones, B, seed=seed)
    deg = np.arange(B) % 2 == 0
    A[deg, 2, :] = A[deg, 0, :]; b[deg, 2] = b[deg, 0]
    keep = oracle.solve_batch(A, b, c, cones, eps=1e-10, max_iters=200000)["status"] == 1
    assert keep.mean() >= 0.8 and deg[keep].sum() >= 4 and (~deg[keep]).sum() >= 4, keep
    return n, cones, A[keep], b[keep], c[keep], deg[keep]


@pytest.mark.parametrize("batch", ["regular", "duplicated_rows"])
def test_backward_of_the_value_launches_no_adjoint(batch):
    from cvxpylayers_amd.torch import CvxpyLayer
    if batch == "regular":
        layer = _layer12(False)
        params = _params12(16, 21)[:3]
        deg = None
    else:
        n, cones, A, b, c, deg = _duplicated_rows_batch()
        layer = CvxpyLayer(template=vk.identity_template(n, cones), solver_args=ref_cases.SOLVER_ARGS)
        params = [_cuda(p).requires_grad_() for p in (A, b, c)]
    eng = layer.ctx.solver_ctx.engine(DEV)
    try:
        for flags, cls, expect in ((4, 1, 0), (4 | 8, 2, None)):
            _lib.check(_lib.lib().ce_set_profiling(eng._h, flags), "ce_set_profiling")
            eng.reset_profile()
            x, y, val = layer(*params, return_value=True)
            eng.reset_profile()
            grads = torch.autograd.grad(val.sum(), params)
            torch.cuda.synchronize()
            launches = eng.profile(cls)[1]
            print("profiling", flags, "class", cls, "launches", launches)
            assert (launches == 0) if expect == 0 else (launches >= 1)
            assert eng.profile(1)[1] == 0
            assert layer.info["adjoint"]["status"] is None
            assert all(torch.isfinite(g_).all() for g_ in grads)
        # the route it replaces launches the adjoint, and flags the duplicated rows 4 | 8
        eng.reset_profile()
        x, y = layer(*params)
        torch.autograd.grad((params[2] * x).sum(), params)
        torch.cuda.synchronize()
        assert eng.profile(1)[1] >= 1
        status = layer.info["adjoint"]["status"].cpu().numpy()
        if deg is not None:
            assert (status[deg] == 12).all() and (status[~deg] == 0).all(), status
    finally:
        eng.set_profiling(0); eng.reset_profile()


# ------------------------------------------------------------------------------------------------ 9. masked instances
def test_a_masked_instance_returns_nan_and_contributes_no_gradient():
    layer, B, bad = _layer12(), 6, 2
    A, b, c = P.generate(N12, CONES12, B, seed=33)
    d = np.random.default_rng(36).standard_normal(B)
    # rows 2 and 3 are nonnegative-cone rows: a^T x <= -1 and -a^T x <= -1 have no common point
    A[bad, 3] = -A[bad, 2]; b[bad, 2] = -1.0; b[bad, 3] = -1.0
    params = [_cuda(p).requires_grad_() for p in (A, b, c, d)]
    args = {"raise_on_error": False}
    x, y, val = layer(*params, solver_args=args, return_value=True)
    status = layer.info["status"].cpu().numpy()
    assert status[bad] < 0 and (np.delete(status, bad) == 1).all(), status
    v = val.detach().cpu().numpy()
    assert np.isnan(v[bad]) and np.isfinite(np.delete(v, bad)).all()
    grads = torch.autograd.grad(torch.nansum(val), params)
    keep = np.arange(B) != bad
    rest = [_cuda(p[keep]).requires_grad_() for p in (A, b, c, d)]
    val_r = layer(*rest, solver_args=args, return_value=True)[-1]
    grads_r = torch.autograd.grad(val_r.sum(), rest)
    assert torch.equal(val.detach()[keep], val_r.detach())
    for name, g_, gr in zip("Abcd", grads, grads_r):
        assert torch.isfinite(g_).all(), name
        assert (g_[bad] == 0).all(), name
        assert torch.equal(g_[keep], gr), name


# ------------------------------------------------------------------------------------------------ 10. gp and objective_sign
@pytest.mark.parametrize("sign", [1, -1])
def test_gp_layers_return_exp_of_the_value_and_maximize_problems_the_maximum(sign):
    """two variables.  sign = 1: minimise 1 / (x y) s.t. x <= a, y <= b -- in log form min -u - v s.t. u <= log a, v <= log b, value 1 / (a b).
    sign = -1: maximise x y under the same constraints: the same canonical program, objective_sign = -1, value a b."""
    from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery
    from cvxpylayers_amd.torch.templates import template_from_affine_builder
    tpl = template_from_affine_builder(lambda la, lb: (np.eye(2), np.array([float(la), float(lb)]), np.array([-1.0, -1.0])), [(), ()], {"z": 0, "l": 2, "q": []},
                                       [VariableRecovery(slice(0, 1), None, ()), VariableRecovery(slice(1, 2), None, ())])
    tpl = dataclasses.replace(tpl, gp=True, gp_log_mask=(True, True), objective_sign=sign)
    layer = CvxpyLayer(template=tpl, solver_args=ref_cases.SOLVER_ARGS)
    a = _cuda(np.array([1.5, 2.0, 0.7])).requires_grad_(); b = _cuda(np.array([0.5, 3.0, 1.1])).requires_grad_()
    xv, yv, val = layer(a, b, return_value=True)
    assert torch.allclose(xv, a.detach(), rtol=1e-6) and torch.allclose(yv, b.detach(), rtol=1e-6)
    want = (a * b) if sign == -1 else 1.0 / (a * b)
    assert torch.allclose(val, want.detach(), rtol=1e-6), (val, want)
    ga, gb = torch.autograd.grad(val.sum(), [a, b])
    wa, wb = torch.autograd.grad(want.sum(), [a, b])
    assert torch.allclose(ga, wa, rtol=1e-6) and torch.allclose(gb, wb, rtol=1e-6)
    assert layer.info["adjoint"]["status"] is None
    # info["objective"] stays the canonical program's: the log-problem's minimum
    assert torch.allclose(layer.info["objective"]["primal"], -(torch.log(a) + torch.log(b)).detach(), atol=1e-6)

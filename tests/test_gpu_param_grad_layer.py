"""solver_args param_grad="factors" through CvxpyLayer on hand-built templates: the parameter gradient from the adjoint's factors (no dA in memory) against the
default dA route of the same layer on the same inputs.

Templates: min c.x + ||x||^2 s.t. F x = g, lo <= x_0 <= 1 (x of six entries returned as a (2, 3) matrix, the multipliers of the equalities as a dual output), once
with parameters (F, g, c, lo) -- A, b and c parameters -- and once with F constant and parameters (g, c, lo): b and c only.  Every parameter entry of both
templates has exactly ONE entry in the transposed parameter maps (asserted), so the bound of tests/test_gpu_param_grad.py -- equality on a row with one map
entry, t 2^-52 sum |val entry| elsewhere -- asks for torch.equal of every Jacobian block and every gradient here; the forward solve is deterministic."""
import warnings

import numpy as np
import pytest
import torch

import kit
from cvxpylayers_amd.interfaces.solver_args import _WARNED
from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery
from cvxpylayers_amd.torch.templates import template_from_affine_builder

pytestmark = pytest.mark.gpu

NX, KEQ, B = 6, 3, 5
ARGS = {"eps": 1e-9, "max_iters": 200000}
KEY = {"param_grad": "factors"}
_F0 = np.random.default_rng(2).standard_normal((KEQ, NX))
_LAYERS: dict = {}


def _rows(F, g, cv, lo):
    k, n = F.shape
    Az = np.zeros((k, n + 1)); Az[:, :n] = F
    Al = np.zeros((2, n + 1)); Al[0, 0] = -1.0; Al[1, 0] = 1.0          # s = x_0 - lo >= 0, s = 1 - x_0 >= 0
    A2, b2 = kit._soc_sumsq_rows(np.eye(n), np.zeros(n), n, n + 1)
    c = np.zeros(n + 1); c[:n] = cv; c[n] = 1.0
    return np.vstack([Az, Al, A2]), np.concatenate([g, [-lo[0], 1.0], b2]), c


def layer_of(kind):
    if kind not in _LAYERS:
        cones = {"z": KEQ, "l": 2, "q": [NX + 2]}
        rec = [VariableRecovery(slice(0, NX), None, (2, 3)), VariableRecovery(None, slice(0, KEQ), (KEQ,), source="dual")]
        if kind == "Abc":
            tpl = template_from_affine_builder(_rows, [(KEQ, NX), (KEQ,), (NX,), (1,)], cones, rec)
        else:
            tpl = template_from_affine_builder(lambda g, cv, lo: _rows(_F0, g, cv, lo), [(KEQ,), (NX,), (1,)], cones, rec)
        layer = CvxpyLayer(template=tpl, solver_args=ARGS)
        terms = np.diff(layer._A.matT.indptr)[:-1] + np.diff(layer._q.matT.indptr)[:-1]
        assert (terms == 1).all(), terms          # one map entry per parameter entry: the derived bound is equality
        _LAYERS[kind] = layer
    return _LAYERS[kind]


def params_of(kind, batched=True, lo=-3.0):
    rng = np.random.default_rng(5)
    F = torch.from_numpy(_F0[None] + 0.1 * rng.standard_normal((B, KEQ, NX))).cuda()
    g = torch.from_numpy(rng.standard_normal((B, KEQ))).cuda()
    cv = torch.from_numpy(0.3 * rng.standard_normal((B, NX))).cuda()
    lov = torch.full((B, 1), lo, dtype=torch.float64).cuda()
    ps = (F, g, cv, lov) if kind == "Abc" else (g, cv, lov)
    return ps if batched else tuple(p[0].clone() for p in ps)


@pytest.mark.parametrize("kind", ["Abc", "bc"])
def test_reverse_jacobian_under_the_key_equals_the_default_in_one_chunk(kind):
    layer = layer_of(kind)
    ps = params_of(kind)
    eng = layer.ctx.solver_ctx.engine(torch.device("cuda", 0))
    assert eng.param_grad_variant >= 0
    per_cot = B * ((eng.m + 1 + eng.n) + (eng.n + 1)) * 8          # what the new route really allocates per cotangent: factor records and dq
    small = NX * per_cot          # room for the six primal cotangents of the new route; the default route's dA rows need several chunks for them
    assert small // (B * eng.nnz_aug * 8) < NX, (small, eng.nnz_aug)
    outs_d, jac_d = layer.jacobian(*ps, max_bytes=small)
    info_d = layer.info
    assert info_d["adjoint"]["path"] == "per_instance" and "param_grad" not in info_d["adjoint"] and info_d["adjoint"]["status"].shape[0] < NX
    calls = []
    orig = eng.vjp_many_params
    eng.vjp_many_params = lambda *a, **k: (calls.append(int(a[4].shape[0])), orig(*a, **k))[1]
    try:
        outs, jac = layer.jacobian(*ps, max_bytes=small, solver_args=KEY)
        info = layer.info
        assert calls == [NX, KEQ], calls
        assert info["adjoint"]["path"] == "ce_vjp_many_params" and info["adjoint"]["param_grad"] == "factors" and eng.last_vjp_many_path == "many_params"
        calls.clear()
        outs_1, jac_1 = layer.jacobian(*ps, max_bytes=1, solver_args=KEY)          # one cotangent per chunk
        assert calls == [1] * (NX + KEQ), calls
    finally:
        eng.vjp_many_params = orig
    for i in range(2):
        assert torch.equal(outs[i], outs_d[i])
        for j in range(len(ps)):
            assert jac[i][j].shape == jac_d[i][j].shape and jac[i][j].dtype == torch.float64
            assert torch.equal(jac[i][j], jac_d[i][j]), (kind, i, j, float((jac[i][j] - jac_d[i][j]).abs().max()))
            assert torch.equal(jac_1[i][j], jac[i][j]), (kind, i, j, "a result depends on the chunk it travelled in")
    assert sum(float(jac[0][j].abs().max()) for j in range(len(ps))) > 1e-3          # (not vacuous)


def _loss_grads(layer, ps, need, **kw):
    ps = [p.clone().requires_grad_(r) for p, r in zip(ps, need)]
    outs = layer(*ps, **kw)
    w = [torch.linspace(0.5, 1.5, o.numel(), dtype=torch.float64, device=o.device).reshape(o.shape) for o in outs]
    loss = sum((o * wi).sum() for o, wi in zip(outs, w))
    loss.backward()
    torch.cuda.synchronize()
    return [o.detach() for o in outs], [p.grad for p in ps], layer.info


@pytest.mark.parametrize("kind", ["Abc", "bc"])
def test_backward_of_a_scalar_loss_under_the_key_equals_the_default(kind):
    layer = layer_of(kind)
    ps = params_of(kind)
    need = [True] * len(ps)
    outs_d, grads_d, info_d = _loss_grads(layer, ps, need)
    assert "param_grad" not in info_d["adjoint"] and info_d["adjoint"]["status"] is not None
    outs, grads, info = _loss_grads(layer, ps, need, solver_args=KEY)
    assert info["adjoint"]["param_grad"] == "factors" and info["adjoint"]["path"] == "per_instance"
    assert torch.equal(info["adjoint"]["status"], info_d["adjoint"]["status"])
    for o, od in zip(outs, outs_d):
        assert torch.equal(o, od)
    for g, gd in zip(grads, grads_d):
        assert g.shape == gd.shape and torch.equal(g, gd), float((g - gd).abs().max())
    assert all(float(gd.abs().max()) > 0 for gd in grads_d[:-1])          # (not vacuous; the bound lo is inactive at these points: its gradient is zero on both routes)
    # a parameter that needs no gradient gets none; warm_start and return_value behave as on the default route
    outs_w, grads_w, _ = _loss_grads(layer, ps, [True] + [False] * (len(ps) - 1), solver_args=KEY, warm_start=True, return_value=True)
    outs_wd, grads_wd, _ = _loss_grads(layer, ps, [True] + [False] * (len(ps) - 1), warm_start=True, return_value=True)
    assert len(outs_w) == 3 and outs_w[2].shape == (B,) and all(g is None for g in grads_w[1:])
    assert torch.allclose(outs_w[2], outs_wd[2], rtol=1e-7, atol=1e-9) and torch.allclose(grads_w[0], grads_wd[0], rtol=1e-5, atol=1e-7)          # (two warm-started solves: not the same iterates)


def test_an_unbatched_parameter_in_a_batched_call_gets_the_gradient_summed_over_the_batch():
    layer = layer_of("bc")
    g, cv, lo = params_of("bc")
    ps = (g, cv[0].clone(), lo)          # c unbatched
    outs_d, grads_d, _ = _loss_grads(layer, ps, [True] * 3)
    outs, grads, info = _loss_grads(layer, ps, [True] * 3, solver_args=KEY)
    assert info["adjoint"]["param_grad"] == "factors" and grads[1].shape == (NX,)
    for gr, gd in zip(grads, grads_d):
        assert torch.equal(gr, gd)
    # and it IS the sum of the per-instance gradients of the batched call
    _, grads_b, _ = _loss_grads(layer, (g, cv[0].expand(B, NX).contiguous(), lo), [True] * 3, solver_args=KEY)
    assert torch.allclose(grads[1], grads_b[1].sum(0), rtol=1e-12, atol=1e-14)
    # fully unbatched call: no batch axis
    up = params_of("bc", batched=False)
    _, gu_d, _ = _loss_grads(layer, up, [True] * 3)
    _, gu, _ = _loss_grads(layer, up, [True] * 3, solver_args=KEY)
    for a, b_ in zip(gu, gu_d):
        assert a.shape == b_.shape and torch.equal(a, b_)


def test_raise_on_error_false_with_one_infeasible_instance_keeps_the_nan_and_zero_pattern():
    layer = layer_of("bc")
    g, cv, lo = params_of("bc")
    lo = lo.clone(); lo[2] = 2.0          # lo > 1: instance 2 is infeasible
    args = {"raise_on_error": False}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        outs_d, grads_d, info_d = _loss_grads(layer, (g, cv, lo), [True] * 3, solver_args=args)
        outs, grads, info = _loss_grads(layer, (g, cv, lo), [True] * 3, solver_args={**args, **KEY})
    assert int(info["status"][2]) < 0 and info["adjoint"]["param_grad"] == "factors"
    for o, od in zip(outs, outs_d):
        assert torch.isnan(o[2]).all() and torch.equal(torch.isnan(o), torch.isnan(od)) and torch.equal(torch.nan_to_num(o), torch.nan_to_num(od))
    for gr, gd in zip(grads, grads_d):
        assert torch.equal(torch.isnan(gr), torch.isnan(gd)) and torch.equal(torch.nan_to_num(gr), torch.nan_to_num(gd))
        assert (gr[2] == 0).all() or torch.isnan(gr[2]).all()
    outs_j, jac = layer.jacobian(g, cv, lo, solver_args={**args, **KEY})
    outs_jd, jac_d = layer.jacobian(g, cv, lo, solver_args=args)
    for i in range(2):
        for j in range(3):
            assert torch.isnan(jac[i][j][2]).all() and torch.equal(torch.isnan(jac[i][j]), torch.isnan(jac_d[i][j]))
            assert torch.equal(torch.nan_to_num(jac[i][j]), torch.nan_to_num(jac_d[i][j]))


def test_an_unserved_template_ignores_the_key_with_one_notice():
    """one PSD block: min tr(C X) s.t. tr X = 1, X PSD (kit.sdp_min_eig), parameter C"""
    k = 3
    d = k * (k + 1) // 2
    def builder(Cm):
        A, b, c = kit.sdp_min_eig(0.5 * (Cm + Cm.T))[:3]
        return A, b, c
    tpl = template_from_affine_builder(builder, [(k, k)], {"z": 1, "l": 0, "q": [], "s": [k]}, [VariableRecovery(slice(0, d), None, (d,))])
    layer = CvxpyLayer(template=tpl, solver_args={"eps": 1e-8, "max_iters": 100000})
    rng = np.random.default_rng(4)
    Cm = torch.from_numpy(rng.standard_normal((3, k, k))).cuda()
    outs_d, grads_d, info_d = _loss_grads(layer, (Cm,), [True])
    _WARNED.discard("param_grad_unserved")
    with pytest.warns(UserWarning, match="param_grad='factors' is not served") as rec:
        outs, grads, info = _loss_grads(layer, (Cm,), [True], solver_args=KEY)
        outs2, grads2, _ = _loss_grads(layer, (Cm,), [True], solver_args=KEY)
        _, jac = layer.jacobian(Cm, solver_args=KEY)
    assert sum("param_grad" in str(w.message) for w in rec) == 1
    assert torch.equal(outs[0], outs_d[0]) and torch.equal(grads[0], grads_d[0]) and torch.equal(grads2[0], grads_d[0])
    assert "param_grad" not in info["adjoint"] and info["adjoint"]["path"] == info_d["adjoint"]["path"] and set(info) == set(info_d)
    _, jac_d = layer.jacobian(Cm)
    assert torch.equal(jac[0][0], jac_d[0][0]) and "param_grad" not in layer.info["adjoint"]


def test_forward_mode_ad_ignores_the_key_with_the_notice():
    import torch.autograd.forward_ad as fwAD
    layer = layer_of("bc")
    g, cv, lo = params_of("bc")
    _WARNED.discard("param_grad_unserved")
    with fwAD.dual_level():
        gd = fwAD.make_dual(g, torch.ones_like(g))
        with pytest.warns(UserWarning, match="forward-mode AD"):
            out = layer(gd, cv, lo, solver_args=KEY)
        t = fwAD.unpack_dual(out[0]).tangent
        out_d = layer(gd, cv, lo)
        assert t is not None and torch.equal(t, fwAD.unpack_dual(out_d[0]).tangent)

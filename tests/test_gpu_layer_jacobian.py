"""CvxpyLayer.jacobian: the Jacobian of every output with respect to every parameter, per instance, from one forward and one many-cotangent adjoint
(interfaces/mi355_if.py adjoint_many -> ConeEngine.vjp_many), against the Jacobian assembled by looping torch.autograd.grad over one-hot cotangents on layer(*params).

The template: min ||x||^2 s.t. F x = g (kit.min_norm_eq) with x of six entries returned as a (2, 3) matrix variable (Fortran reshape, as the frontend recovers it)
and the multipliers of the three equalities as a dual-variable output; parameters F (3, 6) and g (3,); B = 6.  Both sides solve to eps = 1e-9; they agree within
1e-6 relative (max |difference| / (1 + max |reference|) per Jacobian block)."""
import warnings

import numpy as np
import pytest
import torch

import kit
from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery
from cvxpylayers_amd.torch.templates import template_from_affine_builder

pytestmark = pytest.mark.gpu

NX, KEQ, B = 6, 3, 6
ARGS = {"eps": 1e-9, "max_iters": 200000}
_CACHE: dict = {}


def _template():
    def builder(F, g):          # kit.min_norm_eq's rows (its closed form does not exist at the F = 0 the affine probing evaluates)
        k, n = F.shape
        Az = np.zeros((k, n + 1)); Az[:, :n] = F
        A2, b2 = kit._soc_sumsq_rows(np.eye(n), np.zeros(n), n, n + 1)
        c = np.zeros(n + 1); c[n] = 1.0
        return np.vstack([Az, A2]), np.concatenate([g, b2]), c
    cones = {"z": KEQ, "l": 0, "q": [NX + 2]}
    rec = [VariableRecovery(slice(0, NX), None, (2, 3)), VariableRecovery(None, slice(0, KEQ), (KEQ,), source="dual")]
    return template_from_affine_builder(builder, [(KEQ, NX), (KEQ,)], cones, rec)


def _params(batched=True):
    rng = np.random.default_rng(5)
    F = torch.from_numpy(rng.standard_normal((B, KEQ, NX))).cuda(); g = torch.from_numpy(rng.standard_normal((B, KEQ))).cuda()
    return (F, g) if batched else (F[0].clone(), g[0].clone())


def _autograd_jacobian(layer, params, **kw):
    """jac[i][j] by one torch.autograd.grad per output element (a one-hot cotangent on that element of every instance: the instances are independent)"""
    ps = [p.clone().requires_grad_(True) for p in params]
    outs = layer(*ps, **kw)
    batched = ps[0].dim() == 3
    nb = 1 if batched else 0
    jac = []
    for o in outs:
        vshape = tuple(o.shape[nb:])
        size = int(np.prod(vshape))
        rows = [[] for _ in ps]
        for t in range(size):
            oh = torch.zeros_like(o).reshape((o.shape[0], size) if batched else (size,))
            oh[..., t] = 1.0
            gs = torch.autograd.grad(o, ps, grad_outputs=oh.reshape(o.shape), retain_graph=True, allow_unused=True)
            for j, (gj, p) in enumerate(zip(gs, ps)):
                rows[j].append(torch.zeros_like(p) if gj is None else gj)
        blocks = []
        for j, p in enumerate(ps):
            st = torch.stack(rows[j], dim=nb)                      # batch + (size,) + param shape
            blocks.append(st.reshape(tuple(p.shape[:nb]) + vshape + tuple(p.shape[nb:])))
        jac.append(tuple(blocks))
    return tuple(o.detach() for o in outs), tuple(jac)


def _rel(got, want):
    return float((got - want).abs().max() / (1 + want.abs().max()))


def _reference():
    if "ref" not in _CACHE:
        layer = CvxpyLayer(template=_template(), solver_args=ARGS)
        _CACHE["layer"] = layer
        _CACHE["ref"] = _autograd_jacobian(layer, _params())
    return _CACHE["layer"], _CACHE["ref"]


def test_jacobian_against_the_autograd_loop_and_chunking():
    layer, (outs_w, jac_w) = _reference()
    tpl = layer.template
    outs, jac = layer.jacobian(*_params())
    eng = layer.ctx.solver_ctx.engine(torch.device("cuda", 0))
    assert eng.last_vjp_many_path == "many" and layer.info["adjoint"]["status"].shape[1] == B
    assert outs[0].shape == (B, 2, 3) and outs[1].shape == (B, KEQ) and not any(o.requires_grad for o in outs)
    assert jac[0][0].shape == (B, 2, 3, KEQ, NX) and jac[0][1].shape == (B, 2, 3, KEQ) and jac[1][0].shape == (B, KEQ, KEQ, NX) and jac[1][1].shape == (B, KEQ, KEQ)
    for i in range(2):
        assert _rel(outs[i], outs_w[i]) < 1e-6
        for j in range(2):
            assert jac[i][j].dtype == torch.float64 and jac[i][j].device.type == "cuda"
            e = _rel(jac[i][j], jac_w[i][j])
            print(f"jac[{i}][{j}]: {e:.2e} of max {float(jac_w[i][j].abs().max()):.2e}")
            assert e < 1e-6, (i, j, e)
    # chunks of one and of three cotangents (max_bytes in units of one cotangent's dA): a cotangent's result does not depend on the chunk it travels in.  The kernel
    # takes the cotangents one after the other through the same code, and the forward solve is deterministic: bit for bit.
    one = B * eng.nnz_aug * 8
    for k_chunk in (1, 3):
        _, jc = layer.jacobian(*_params(), max_bytes=k_chunk * one)
        for i in range(2):
            for j in range(2):
                assert torch.equal(jc[i][j], jac[i][j]), (k_chunk, i, j, _rel(jc[i][j], jac[i][j]))


def test_unbatched_call_has_no_batch_axis():
    layer, _ = _reference()
    F, g = _params(batched=False)
    outs, jac = layer.jacobian(F, g)
    assert outs[0].shape == (2, 3) and outs[1].shape == (KEQ,)
    assert jac[0][0].shape == (2, 3, KEQ, NX) and jac[0][1].shape == (2, 3, KEQ) and jac[1][0].shape == (KEQ, KEQ, NX) and jac[1][1].shape == (KEQ, KEQ)
    _, jac_w = _autograd_jacobian(layer, (F, g))
    for i in range(2):
        for j in range(2):
            assert _rel(jac[i][j], jac_w[i][j]) < 1e-6, (i, j)


def test_unbatched_parameter_in_a_batched_call_is_differentiated_per_instance():
    layer, _ = _reference()
    F, g = _params()
    outs, jac = layer.jacobian(F, g[0])
    assert jac[0][1].shape == (B, 2, 3, KEQ) and jac[1][1].shape == (B, KEQ, KEQ)
    _, jac_w = _autograd_jacobian(layer, (F, g[0].expand(B, KEQ).contiguous()))          # its expanded copy
    for i in range(2):
        for j in range(2):
            assert _rel(jac[i][j], jac_w[i][j]) < 1e-6, (i, j)


def test_an_infeasible_instance_returns_nan_rows_and_leaves_the_others_alone():
    layer, (_, jac_w) = _reference()
    F, g = _params()
    bad = 2
    F = F.clone(); g = g.clone()
    F[bad, 1] = F[bad, 0]; g[bad, 1] = g[bad, 0] + 1.0                 # two equalities that contradict each other
    with warnings.catch_warnings():          # (the outcome of an asynchronous forward is reported as warnings, if at all)
        warnings.simplefilter("ignore")
        outs, jac = layer.jacobian(F, g, solver_args={"raise_on_error": False})
    torch.cuda.synchronize()
    good = [i for i in range(B) if i != bad]
    for i in range(2):
        assert torch.isnan(outs[i][bad]).all()
        for j in range(2):
            assert torch.isnan(jac[i][j][bad]).all(), (i, j)
            assert torch.isfinite(jac[i][j][good]).all()
            assert _rel(jac[i][j][good], jac_w[i][j][good]) < 1e-6, (i, j)


def test_a_native_quadratic_objective_returns_the_P_parameter_jacobian_through_the_loop():
    n = 5

    def builder(Pp, qp):
        A = np.zeros((1 + n, n)); b = np.zeros(1 + n)
        A[0] = 1.0; b[0] = 1.0
        A[1:] = -np.eye(n)
        return A, b, qp, 0.5 * (Pp + Pp.T)
    tpl = template_from_affine_builder(builder, [(n, n), (n,)], {"z": 1, "l": n, "q": [], "s": []}, [VariableRecovery(slice(0, n), None, (n,))])
    layer = CvxpyLayer(template=tpl, solver_args={"eps": 1e-10, "max_iters": 200000})
    torch.manual_seed(3)
    G = torch.randn(4, n, n, dtype=torch.float64, device="cuda")
    Pt = G @ G.transpose(1, 2) / n + torch.eye(n, dtype=torch.float64, device="cuda")
    qt = 0.1 * torch.randn(4, n, dtype=torch.float64, device="cuda")
    outs, jac = layer.jacobian(Pt, qt)
    eng = layer.ctx.solver_ctx.engine(torch.device("cuda", 0))
    assert eng.qp_native and eng.last_vjp_many_path == "loop"
    assert jac[0][0].shape == (4, n, n, n) and jac[0][1].shape == (4, n, n)
    _, jac_w = _autograd_jacobian(layer, (Pt, qt))
    assert float(jac_w[0][0].abs().max()) > 1e-3
    for j in range(2):
        e = _rel(jac[0][j], jac_w[0][j])
        print(f"QP-native jac[0][{j}]: {e:.2e}")
        assert e < 1e-6, (j, e)

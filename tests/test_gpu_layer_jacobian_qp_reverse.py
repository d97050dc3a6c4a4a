"""CvxpyLayer.jacobian in the reverse direction on a layer whose quadratic objective runs inside the kernels, under solver_args qp_adjoint="search_free": one
ce_vjp_qp_many call per chunk (each instance factored once, dP among the outputs) instead of the loop of ce_vjp_qp calls.

The n = 5 layer of test_gpu_layer_jacobian.py::test_a_native_quadratic_objective_returns_the_P_parameter_jacobian_through_the_loop (min 1/2 x^T P x + q^T x on the
simplex, parameters P (5, 5) and q (5,), B = 4).  Same shapes as the default route; agreement with the default loop Jacobian and with the torch.autograd.grad
Jacobian within 1e-6 relative (that file's bound); without the key the loop still runs; a max_bytes that forces several chunks changes nothing."""
import numpy as np
import pytest
import torch

from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery
from cvxpylayers_amd.torch.templates import template_from_affine_builder
from test_gpu_layer_jacobian import _autograd_jacobian, _rel

pytestmark = pytest.mark.gpu

N, B = 5, 4
SEARCH_FREE = {"qp_adjoint": "search_free"}
_CACHE: dict = {}


def _setup():
    """the layer, its parameters, and the three Jacobians every test compares: computed once, shared, not changed"""
    if _CACHE:
        return _CACHE
    n = N

    def builder(Pp, qp):
        A = np.zeros((1 + n, n)); b = np.zeros(1 + n)
        A[0] = 1.0; b[0] = 1.0
        A[1:] = -np.eye(n)
        return A, b, qp, 0.5 * (Pp + Pp.T)
    tpl = template_from_affine_builder(builder, [(n, n), (n,)], {"z": 1, "l": n, "q": [], "s": []}, [VariableRecovery(slice(0, n), None, (n,))])
    layer = CvxpyLayer(template=tpl, solver_args={"eps": 1e-10, "max_iters": 200000})
    torch.manual_seed(3)
    G = torch.randn(B, n, n, dtype=torch.float64, device="cuda")
    Pt = G @ G.transpose(1, 2) / n + torch.eye(n, dtype=torch.float64, device="cuda")
    qt = 0.1 * torch.randn(B, n, dtype=torch.float64, device="cuda")
    eng = layer.ctx.solver_ctx.engine(torch.device("cuda", 0))
    outs_l, jac_l = layer.jacobian(Pt, qt)
    path_l, info_l = eng.last_vjp_many_path, dict(layer.info["adjoint"])
    outs_s, jac_s = layer.jacobian(Pt, qt, solver_args=SEARCH_FREE)
    path_s, kernel_s, info_s = eng.last_vjp_many_path, eng.last_vjp_kernel, dict(layer.info["adjoint"])
    _, jac_w = _autograd_jacobian(layer, (Pt, qt))
    _CACHE.update(layer=layer, eng=eng, params=(Pt, qt), loop=(outs_l, jac_l, path_l, info_l), sf=(outs_s, jac_s, path_s, kernel_s, info_s), autograd=jac_w)
    return _CACHE


def test_the_search_free_reverse_jacobian_runs_many_and_agrees_with_the_loop_and_autograd():
    c = _setup()
    outs_l, jac_l, path_l, info_l = c["loop"]
    outs_s, jac_s, path_s, kernel_s, info_s = c["sf"]
    assert c["eng"].qp_native
    assert path_s == "many" and kernel_s == "ce_vjp_qp_many" and info_s["path"] == "ce_vjp_qp_many"
    st = info_s["status"]
    assert tuple(st.shape) == (N, B) and (st.cpu().numpy() == 0).all(), st
    assert torch.equal(outs_s[0], outs_l[0])
    assert jac_s[0][0].shape == jac_l[0][0].shape == (B, N, N, N) and jac_s[0][1].shape == jac_l[0][1].shape == (B, N, N)
    assert float(c["autograd"][0][0].abs().max()) > 1e-3
    for j in range(2):
        el, ew = _rel(jac_s[0][j], jac_l[0][j]), _rel(jac_s[0][j], c["autograd"][0][j])
        print(f"search-free jac[0][{j}]: against the loop {el:.2e}, against autograd {ew:.2e}")
        assert el < 1e-6 and ew < 1e-6, (j, el, ew)


def test_without_the_key_the_loop_still_runs():
    c = _setup()
    _, _, path_l, info_l = c["loop"]
    assert path_l == "loop" and info_l["path"] != "ce_vjp_qp_many"
    layer, eng = c["layer"], c["eng"]
    layer.jacobian(*c["params"], solver_args={"qp_adjoint": "pivoting"})
    assert eng.last_vjp_many_path == "loop" and eng.last_vjp_kernel is None


def test_several_chunks_give_the_one_chunk_result():
    c = _setup()
    layer, eng = c["layer"], c["eng"]
    per_cotangent = B * (eng.nnz_aug + eng.nnz_p) * 8          # the chunk's dA and dP
    calls = []
    orig = eng.vjp_many
    eng.vjp_many = lambda *a, **kw: (calls.append(int(a[4].shape[0])), orig(*a, **kw))[1]
    try:
        _, jac_c = layer.jacobian(*c["params"], solver_args=SEARCH_FREE, max_bytes=2 * per_cotangent)
    finally:
        del eng.vjp_many
    assert calls == [2, 2, 1] and eng.last_vjp_kernel == "ce_vjp_qp_many", calls
    # a max_bytes that holds two cotangents' dA but not their dP as well: one cotangent per chunk
    calls.clear()
    eng.vjp_many = lambda *a, **kw: (calls.append(int(a[4].shape[0])), orig(*a, **kw))[1]
    try:
        layer.jacobian(*c["params"], solver_args=SEARCH_FREE, max_bytes=2 * B * eng.nnz_aug * 8)
    finally:
        del eng.vjp_many
    assert eng.nnz_p > 0 and calls == [1] * N, calls
    for j in range(2):
        assert torch.equal(jac_c[0][j], c["sf"][1][0][j]), j


def test_backward_ignores_the_key():
    c = _setup()
    layer, eng = c["layer"], c["eng"]
    Pt, qt = (p.clone().requires_grad_(True) for p in c["params"])
    (x,) = layer(Pt, qt, solver_args=SEARCH_FREE)
    eng.last_vjp_kernel = "untouched"
    x.sum().backward()
    assert eng.last_vjp_kernel == "untouched" and Pt.grad is not None and layer.info["adjoint"]["path"] != "ce_vjp_qp_many"

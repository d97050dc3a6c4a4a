"""CvxpyLayer.jacobian(direction="forward"): the Jacobian by columns -- one tangent per parameter entry, the columns of the forward parameter maps handed over once for
the whole batch (stride 0), through interfaces/mi355_if.py tangent_many -> ConeEngine.jvp_many -- against direction="reverse" (test_gpu_layer_jacobian.py's subject,
itself checked against the autograd loop there) on that file's layers: 1e-6 relative (max |difference| / (1 + max |reference|) per Jacobian block).  Chunking is
bit-identical, "auto" picks the direction with fewer right-hand sides, the default call is bit-identical to direction="reverse"."""
import warnings

import numpy as np
import pytest
import torch

import kit
from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery
from cvxpylayers_amd.torch.templates import template_from_affine_builder
from test_gpu_layer_jacobian import ARGS, B, KEQ, NX, _params, _rel, _template

pytestmark = pytest.mark.gpu

_CACHE: dict = {}
DEV = torch.device("cuda", 0)


def _layer():
    if "layer" not in _CACHE:
        layer = CvxpyLayer(template=_template(), solver_args=ARGS)
        _CACHE["layer"] = layer
        _CACHE["reverse"] = layer.jacobian(*_params(), direction="reverse")
    return _CACHE["layer"], _CACHE["reverse"]


def _engine(layer):
    return layer.ctx.solver_ctx.engine(DEV)


def test_forward_against_reverse_and_chunking():
    layer, (outs_w, jac_w) = _layer()
    eng = _engine(layer)
    eng.last_jvp_many_path = eng.last_vjp_many_path = None
    outs, jac = layer.jacobian(*_params(), direction="forward")
    assert eng.last_jvp_many_path == "many" and eng.last_vjp_many_path is None
    st = layer.info["jvp"]["status"]
    assert st.shape[1] == B and layer.info["jvp"]["iters"].shape == st.shape and layer.info["jvp"]["path"] == "direct"
    for i in range(2):
        assert torch.equal(outs[i], outs_w[i])
        for j in range(2):
            assert jac[i][j].shape == jac_w[i][j].shape and jac[i][j].dtype == torch.float64 and jac[i][j].device.type == "cuda"
            e = _rel(jac[i][j], jac_w[i][j])
            print(f"forward against reverse jac[{i}][{j}]: {e:.2e} of max {float(jac_w[i][j].abs().max()):.2e}")
            assert e < 1e-6, (i, j, e)
    # chunks of one and of four tangents (max_bytes in units of one tangent's dx, dy, ds): a tangent's result does not depend on the chunk it travels in
    one = B * (eng.n + 2 * eng.m) * 8
    for c_chunk in (1, 4):
        _, jc = layer.jacobian(*_params(), direction="forward", max_bytes=c_chunk * one)
        for i in range(2):
            for j in range(2):
                assert torch.equal(jc[i][j], jac[i][j]), (c_chunk, i, j, _rel(jc[i][j], jac[i][j]))


def test_the_default_call_is_the_reverse_direction_bit_for_bit():
    layer, (outs_w, jac_w) = _layer()
    eng = _engine(layer)
    eng.last_jvp_many_path = eng.last_vjp_many_path = None
    outs, jac = layer.jacobian(*_params())
    assert eng.last_vjp_many_path == "many" and eng.last_jvp_many_path is None
    for i in range(2):
        assert torch.equal(outs[i], outs_w[i])
        for j in range(2):
            assert torch.equal(jac[i][j], jac_w[i][j]), (i, j)


def test_unbatched_call_has_no_batch_axis():
    layer, _ = _layer()
    F, g = _params(batched=False)
    _, jac_w = layer.jacobian(F, g, direction="reverse")
    outs, jac = layer.jacobian(F, g, direction="forward")
    assert outs[0].shape == (2, 3) and outs[1].shape == (KEQ,)
    assert jac[0][0].shape == (2, 3, KEQ, NX) and jac[0][1].shape == (2, 3, KEQ) and jac[1][0].shape == (KEQ, KEQ, NX) and jac[1][1].shape == (KEQ, KEQ)
    for i in range(2):
        for j in range(2):
            assert _rel(jac[i][j], jac_w[i][j]) < 1e-6, (i, j)


def test_an_infeasible_instance_returns_nan_rows_and_leaves_the_others_alone():
    layer, (_, jac_ref) = _layer()
    F, g = _params()
    bad = 2
    F = F.clone(); g = g.clone()
    F[bad, 1] = F[bad, 0]; g[bad, 1] = g[bad, 0] + 1.0                 # two equalities that contradict each other
    with warnings.catch_warnings():          # (the outcome of an asynchronous forward is reported as warnings, if at all)
        warnings.simplefilter("ignore")
        _, jac_w = layer.jacobian(F, g, solver_args={"raise_on_error": False}, direction="reverse")
        outs, jac = layer.jacobian(F, g, solver_args={"raise_on_error": False}, direction="forward")
    torch.cuda.synchronize()
    good = [i for i in range(B) if i != bad]
    for i in range(2):
        assert torch.isnan(outs[i][bad]).all()
        for j in range(2):
            assert torch.isnan(jac[i][j][bad]).all(), (i, j)
            assert torch.isfinite(jac[i][j][good]).all()
            assert _rel(jac[i][j][good], jac_w[i][j][good]) < 1e-6, (i, j)
            assert _rel(jac[i][j][good], jac_ref[i][j][good]) < 1e-6, (i, j)


def test_a_native_quadratic_objective_gets_its_P_parameter_jacobian_from_one_factorisation():
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
    _, jac_w = layer.jacobian(Pt, qt, direction="reverse")
    eng = _engine(layer)
    assert eng.qp_native and eng.last_vjp_many_path == "loop"
    outs, jac = layer.jacobian(Pt, qt, direction="forward")
    assert eng.last_jvp_many_path == "many" and eng.last_jvp_kernel == "ce_jvp_qp_many"
    assert jac[0][0].shape == (4, n, n, n) and jac[0][1].shape == (4, n, n) and float(jac_w[0][0].abs().max()) > 1e-3
    for j in range(2):
        e = _rel(jac[0][j], jac_w[0][j])
        print(f"QP-native forward against reverse jac[0][{j}]: {e:.2e}")
        assert e < 1e-6, (j, e)


def _two_parameter_layer():
    """min ||x||^2 s.t. (F0 + a F1) x = g0 + b h0 with two scalar parameters a, b (one in A: the layer has per-instance matrices) and the six entries of x as the
    output: 2 parameter entries, 6 output elements"""
    rng = np.random.default_rng(8)
    F0, F1, g0, h0 = rng.standard_normal((KEQ, NX)), rng.standard_normal((KEQ, NX)), rng.standard_normal(KEQ), rng.standard_normal(KEQ)

    def builder(a, b):
        Az = np.zeros((KEQ, NX + 1)); Az[:, :NX] = F0 + a[0] * F1
        A2, b2 = kit._soc_sumsq_rows(np.eye(NX), np.zeros(NX), NX, NX + 1)
        c = np.zeros(NX + 1); c[NX] = 1.0
        return np.vstack([Az, A2]), np.concatenate([g0 + b[0] * h0, b2]), c
    tpl = template_from_affine_builder(builder, [(1,), (1,)], {"z": KEQ, "l": 0, "q": [NX + 2]}, [VariableRecovery(slice(0, NX), None, (NX,))])
    return CvxpyLayer(template=tpl, solver_args=ARGS)


def test_auto_picks_the_direction_with_fewer_right_hand_sides():
    two = _two_parameter_layer()
    rng = np.random.default_rng(9)
    a, b = (torch.from_numpy(0.2 * rng.random((B, 1))).cuda() for _ in range(2))
    _, jac_r = two.jacobian(a, b, direction="reverse")
    eng = _engine(two)
    eng.last_jvp_many_path = eng.last_vjp_many_path = None
    _, jac = two.jacobian(a, b, direction="auto")
    assert eng.last_jvp_many_path == "many" and eng.last_vjp_many_path is None          # 2 parameter entries < 6 output elements: forward
    assert jac[0][0].shape == (B, NX, 1) and jac[0][1].shape == (B, NX, 1) and float(jac_r[0][0].abs().max()) > 1e-3
    for j in range(2):
        assert _rel(jac[0][j], jac_r[0][j]) < 1e-6, j
    layer, (_, jac_w) = _layer()          # 21 parameter entries, 9 output elements: reverse
    eng = _engine(layer)
    eng.last_jvp_many_path = eng.last_vjp_many_path = None
    _, jac = layer.jacobian(*_params(), direction="auto")
    assert eng.last_vjp_many_path == "many" and eng.last_jvp_many_path is None
    assert all(torch.equal(jac[i][j], jac_w[i][j]) for i in range(2) for j in range(2))


def test_an_explicit_jvp_mode_lsqr_runs_the_loop_of_lsqr_solves():
    layer, (_, jac_w) = _layer()
    eng = _engine(layer)
    _, jac = layer.jacobian(*_params(), direction="forward", solver_args={"jvp_mode": "lsqr"})
    assert eng.last_jvp_many_path == "loop" and layer.info["jvp"]["path"] == "lsqr" and (layer.info["jvp"]["iters"] > 0).all()
    assert all(torch.isfinite(jac[i][j]).all() and jac[i][j].shape == jac_w[i][j].shape for i in range(2) for j in range(2))

"""solver_args forward_kernel="wave" through CvxpyLayer on hand-built templates: the forward solve by k_fwd_wave (one instance per wave) against the default route of the
same layer on the same inputs, forward and backward.  Served layer: n = 16, z 2, l 10, q [4, 16] with parameters (A, b, c), eps 1e-8, B = 16 -- outputs within the parity
tolerance max(1e-6, 20 eps) (1 + |.|_inf), parameter gradients within 1e-5 relative; the same with warm_start=True on a second call and with raise_on_error=False.
Without the key info has no "forward" entry.  A layer the kernel does not serve (one exponential cone) ignores the key with one notice: outputs and gradients equal."""
import warnings

import numpy as np
import pytest
import torch

import kit
from cvxpylayers_amd import problems as P
from cvxpylayers_amd.interfaces.solver_args import _WARNED
from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery
from cvxpylayers_amd.torch.templates import template_from_affine_builder

pytestmark = pytest.mark.gpu

N, CONES, B, EPS = 16, dict(z=2, l=10, q=[4, 16]), 16, 1e-8
M = P.cone_rows(CONES)
ARGS = {"eps": EPS, "max_iters": 20000}
KEY = {"forward_kernel": "wave"}
_LAYERS: dict = {}


def served_layer():
    if "served" not in _LAYERS:
        rec = [VariableRecovery(slice(0, N), None, (N,)), VariableRecovery(None, slice(0, M), (M,), source="dual")]
        tpl = template_from_affine_builder(lambda A, b, c: (A, b, c), [(M, N), (M,), (N,)], CONES, rec)
        _LAYERS["served"] = CvxpyLayer(template=tpl, solver_args=ARGS)
    return _LAYERS["served"]


def exp_layer():
    """entropy maximisation over the simplex of mass g (kit.entropy_max): one parameter in b, exponential cones -- not the wave kernel's"""
    if "exp" not in _LAYERS:
        A0, b0, c0, cones, _ = kit.entropy_max(2)

        rec = [VariableRecovery(slice(0, 2), None, (2,))]
        tpl = template_from_affine_builder(lambda g: (A0, b0 + np.eye(len(b0))[0] * (g[0] - b0[0]), c0), [(1,)], cones, rec)
        _LAYERS["exp"] = CvxpyLayer(template=tpl, solver_args={"eps": 1e-8, "max_iters": 100000})
    return _LAYERS["exp"]


def params():
    A, b, c = P.generate(N, CONES, B, seed=5)
    return tuple(torch.from_numpy(v).cuda().requires_grad_(True) for v in (A, b, c))


def run(layer, ps, **kw):
    """forward + backward of a scalar loss; (outputs, parameter gradients, info)"""
    for p in ps:
        p.grad = None
    outs = layer(*ps, **kw)
    info = layer.info
    w = [torch.linspace(0.5, 1.5, o[0].numel(), dtype=torch.float64, device=o.device).reshape(o[0].shape) for o in outs]
    sum(((o * wi) ** 2).sum() + (o * wi).sum() for o, wi in zip(outs, w)).backward()
    torch.cuda.synchronize()
    return [o.detach().cpu().numpy() for o in outs], [p.grad.detach().cpu().numpy().copy() for p in ps], info


def close(got, want):
    outs, grads, _ = got
    outs0, grads0, _ = want
    tol = max(1e-6, 20 * EPS)
    for o, o0 in zip(outs, outs0):
        err = np.abs(o - o0).reshape(B, -1).max(axis=1) / (1 + np.abs(o0).reshape(B, -1).max(axis=1))
        print(f"outputs: max err {err.max():.3e} (tol {tol:.1e})")
        assert err.max() < tol, err.max()
    for g, g0 in zip(grads, grads0):
        rel = np.abs(g - g0).max() / (1 + np.abs(g0).max())
        print(f"gradient {g.shape}: {rel:.3e} (bound 1e-5)")
        assert rel < 1e-5, rel


def test_forward_and_backward_under_the_key_against_the_default_route():
    layer, ps = served_layer(), params()
    base = run(layer, ps)
    assert "forward" not in base[2]          # a served layer without the key: no such entry
    got = run(layer, ps, solver_args=KEY)
    assert got[2]["forward"] == {"kernel": "k_fwd_wave"}
    assert (got[2]["status"].cpu().numpy() == 1).all() and (base[2]["status"].cpu().numpy() == 1).all()
    assert np.abs(got[2]["iters"].cpu().numpy().astype(int) - base[2]["iters"].cpu().numpy().astype(int)).max() <= 25
    close(got, base)
    eng = layer.ctx.solver_ctx.engine(torch.device("cuda", 0))
    assert eng.wave_plan()[0] >= 0 and eng.last_forward_kernel == "k_fwd_wave"
    again = run(layer, ps)
    assert "forward" not in again[2] and eng.last_forward_kernel is None
    for a_, b_ in zip(again[0] + again[1], base[0] + base[1]):          # the key leaves nothing behind: the default route gives its bits again
        assert np.array_equal(a_, b_)


def test_warm_start_on_a_second_call():
    layer, ps = served_layer(), params()
    run(layer, ps)
    base = run(layer, ps, warm_start=True)
    cold = run(layer, ps, solver_args=KEY)
    got = run(layer, ps, solver_args=KEY, warm_start=True)
    assert got[2]["forward"] == {"kernel": "k_fwd_wave"}
    assert got[2]["iters"].cpu().numpy().mean() < cold[2]["iters"].cpu().numpy().mean()
    assert np.abs(got[2]["iters"].cpu().numpy().astype(int) - base[2]["iters"].cpu().numpy().astype(int)).max() <= 25
    close(got, base)


def test_raise_on_error_false():
    layer, ps = served_layer(), params()
    base = run(layer, ps, solver_args={"raise_on_error": False})
    got = run(layer, ps, solver_args={**KEY, "raise_on_error": False})
    assert got[2]["forward"] == {"kernel": "k_fwd_wave"} and "forward" not in base[2]
    close(got, base)


def test_unserved_layer_ignores_the_key_with_one_notice():
    layer = exp_layer()
    g = torch.linspace(0.4, 0.9, B, dtype=torch.float64).reshape(B, 1).cuda().requires_grad_(True)
    base = run(layer, (g,))
    assert "forward" not in base[2]
    _WARNED.discard("forward_kernel_none")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        got = run(layer, (g,), solver_args=KEY)
        got2 = run(layer, (g,), solver_args=KEY)
    assert len([w for w in rec if "forward_kernel" in str(w.message)]) == 1, [str(w.message) for w in rec]
    assert got[2]["forward"] == {"kernel": "workgroup"} == got2[2]["forward"]
    eng = layer.ctx.solver_ctx.engine(torch.device("cuda", 0))
    assert eng.wave_plan() == (-1, 0)
    for a_, b_ in zip(got[0] + got[1] + got2[0] + got2[1], (base[0] + base[1]) * 2):
        assert np.array_equal(a_, b_)

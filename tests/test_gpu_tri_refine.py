"""Newton refinement on templates with exponential / power triples: k_backward_ns<..., FWD, REF, TRI> behind ce_refine (ce_tri_ns_variant >= 0),
ConeEngine.refine, solver_args refine_steps.  The recipes of test_gpu_refine.py on three shapes of tri_ns_kit.SHAPES, with the dense D of a triple from the
oracle: the starting point is the engine's own solve at eps = 1e-4 (once per shape, never changed).  Checked against the direct forward derivative fed the
residual, a dense numpy Newton step, the safeguard (never worse, from the eps = 1e-4 point and from a 25-iteration start), the oracle's eps = 1e-10 point, and
through the layer (refine_steps without a warning, backward at the refined point, forward_ad with jvp_mode="direct")."""
import warnings

import numpy as np
import pytest
import torch
import torch.autograd.forward_ad as fwAD

import notebook_cases as nc
import tri_ns_kit as K
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR
from test_gpu_refine import _assert_never_worse, _check_step_bounds, _refine, _solve_start, _step_errors

pytestmark = pytest.mark.gpu

NAMES = ["exp_small", "exp_pow_mixed", "E"]
_CACHE: dict = {}


def _shape(name):
    """the shape's problem, its eps = 1e-4 start on the GPU, one and three refinement steps from it and the oracle's eps = 1e-10 point: once, shared, not changed"""
    if name not in _CACHE:
        n, cones, A, b, c, hi = K.problem(name)
        r = _solve_start(P.dense_template(n, cones), A, b, c)
        assert _lib.lib().ce_tri_ns_variant(r["eng"]._h) == K.SHAPES[name][4]
        r["cones"], r["hi"] = cones, hi
        r["one"], r["three"] = _refine(r, 1), _refine(r, 3)          # (asserts info["path"] == "ns": what a plain-cone template reports)
        _CACHE[name] = r
    return _CACHE[name]


def _solved(r):
    return r["status"].cpu().numpy() >= 0


@pytest.mark.parametrize("shape", NAMES)
def test_one_step_is_the_direct_jvp_with_the_residual_as_tangent(shape):
    r = _shape(shape)
    tpl, eng, A, b, c = r["tpl"], r["eng"], r["A"], r["b"], r["c"]
    x0, y0, s0 = r["np"]
    B = x0.shape[0]
    gx = np.zeros((B, tpl.n)); gy = np.zeros((B, tpl.m))
    for i in range(B):
        fx, fy, _, _ = K.residual(A[i], b[i], c[i], x0[i], y0[i] - s0[i], r["cones"])
        gx[i], gy[i] = fx, -fy
    tA = np.zeros((B, tpl.nnz_aug)); tA[:, tpl.nnzA + np.arange(tpl.b_idx.size)] = gy[:, tpl.b_idx]
    tq = np.zeros((tpl.n + 1, B)); tq[:tpl.n] = gx.T
    dx, dy, ds, jst = eng.jvp(r["A_bm"], *r["pt"], torch.from_numpy(tA).cuda(), torch.from_numpy(tq).cuda(), path="per_instance", lsqr=TIGHT_LSQR, q_eval=r["q_t"], method="direct")
    assert eng.last_jvp_kernel == "ce_jvp"
    torch.cuda.synchronize()
    dx, dy, ds, jst = (t.cpu().numpy() for t in (dx, dy, ds, jst))
    st = r["one"][3]
    kept = (st & 1) != 0
    print("kept", kept.mean(), "refine status counts", np.bincount(st), "jvp status counts", np.bincount(jst))
    assert kept.mean() >= 0.9
    # the same elimination flags the same instances -- but for the ones the forward derivative alone hands to its re-solve for accuracy (a weighted triple row with
    # 1 - lambda < 1e-5, csrc/ce_backward_ns.h NS_TRI_STIFF): a Newton step takes those, so a flagged derivative may stand beside a kept step, never the reverse
    assert ((jst != 0) | ((st & 4) == 0))[_solved(r)].all()
    both = kept & (jst == 0)
    assert both.mean() >= 0.8
    _check_step_bounds(_step_errors(r, dx, dy - ds, both), "one step vs ce_jvp")


@pytest.mark.parametrize("shape", NAMES)
def test_one_step_is_a_dense_newton_step(shape):
    r = _shape(shape)
    A, b, c, cones = r["A"], r["b"], r["c"], r["cones"]
    x0, y0, s0 = r["np"]
    v0 = y0 - s0
    dxr, dvr, ok = K.dense_newton(A, b, c, x0, v0, cones)
    B = x0.shape[0]
    acc = np.zeros(B, bool)
    for i in np.flatnonzero(ok):
        fx, fy, _, _ = K.residual(A[i], b[i], c[i], x0[i], v0[i], cones)
        fxn, fyn, _, _ = K.residual(A[i], b[i], c[i], x0[i] + dxr[i], v0[i] + dvr[i], cones)
        acc[i] = max(np.abs(fxn).max(), np.abs(fyn).max()) < max(np.abs(fx).max(), np.abs(fy).max())
    st = r["one"][3]
    kept = (st & 1) != 0
    print("well conditioned", ok.mean(), "reference accepts", acc[ok].mean(), "kernel kept", kept[ok].mean())
    both = ok & acc & kept
    assert both.mean() >= 0.8, both.mean()
    _check_step_bounds(_step_errors(r, dxr, dvr, both), "one step vs numpy")


@pytest.mark.parametrize("shape", NAMES)
@pytest.mark.parametrize("steps", ["one", "three"])
def test_never_worse(shape, steps):
    r = _shape(shape)
    st = _assert_never_worse(r["np"], r[steps])
    solved = _solved(r)
    assert (((st & 16) == 0) == solved).all() and ((st[solved] & 7) != 0).all()          # failed instances are skipped; every other one took a step, was rejected or was flagged
    rn = K.rho(r["A"], r["b"], r["c"], *r[steps][:3])
    r0 = r[steps][5]
    assert (rn <= r0 * (1 + 1e-9) + 1e-15)[solved].all()          # rho recomputed in extended precision agrees that nothing grew


@pytest.mark.parametrize("shape", NAMES)
def test_three_steps_land_closer_to_the_oracle_point(shape):
    """distance of the whole point (x, y, s) to the oracle's eps = 1e-10 point, max norm: smaller after three steps than before on every instance the forward
    solve did not fail on"""
    r = _shape(shape)
    hi = r["hi"]
    solved = _solved(r) & (hi["status"] == 1)
    assert solved.mean() >= 0.9
    def dist(pt):
        return np.max([np.abs(g - hi[k]).max(axis=1) for g, k in zip(pt, "xys")], axis=0)
    d0, d3 = dist(r["np"]), dist(r["three"][:3])
    st, r0, r1 = r["three"][3], r["three"][5], r["three"][6]
    print(f"{shape}: status counts {np.bincount(st)}; resid before median {np.nanmedian(r0):.2e}, after median {np.nanmedian(r1):.2e} max {np.nanmax(r1):.2e}; "
          f"distance before median {np.median(d0[solved]):.2e} max {d0[solved].max():.2e}, after median {np.median(d3[solved]):.2e} max {d3[solved].max():.2e}; "
          f"not closer: {np.flatnonzero(solved & ~(d3 < d0))}")
    assert (d3 < d0)[solved].all(), (d0, d3, st)


def test_never_worse_from_a_25_iteration_start():
    n, cones, A, b, c, _ = K.problem("E")
    r = _solve_start(P.dense_template(n, cones), A, b, c, max_iters=25)
    out = _refine(r, 3, status=None)
    st = _assert_never_worse(r["np"], out)
    print("status counts", np.bincount(st), "resid before median", np.median(out[5]), "after median", np.median(out[6]))
    assert ((st & 16) == 0).all()
    rn = K.rho(A, b, c, *out[:3])
    assert (rn <= out[5] * (1 + 1e-9) + 1e-15).all()


def _resource_inputs():
    rng = np.random.default_rng(0)
    m, B = 10, 16
    alpha = rng.uniform(0.1, 0.9, m); Pm = rng.uniform(0.05, 1.0, (B, m)); budget = rng.uniform(0.5, 10.0, B)
    return m, B, [budget, 1.0 / Pm, alpha]


def _oracle_reference(tpl_builder_inputs, w):
    """the oracle's eps = 1e-10 point of the resource-allocation instances and its dense adjoint of sum(w * y) there, as gradients of the three parameters"""
    from oracle import oracle
    m, B, (budget, invp, alpha) = tpl_builder_inputs
    cones = dict(z=1 + m, l=m, q=[], s=[], ep=m)
    nv, rows = 3 * m, 1 + 5 * m
    A = np.zeros((B, rows, nv)); rhs = np.zeros((B, rows)); c = np.zeros((B, nv)); c[:, 2 * m:] = -1.0
    A[:, 0, :m] = 1.0; rhs[:, 0] = budget
    for i in range(m):
        A[:, 1 + i, m + i] = 1.0; A[:, 1 + i, i] = -invp[:, i]
        A[:, 1 + m + i, i] = -1.0
        r0 = 1 + 2 * m + 3 * i
        A[:, r0, m + i] = alpha[i]; rhs[:, r0 + 1] = 1.0; A[:, r0 + 2, 2 * m + i] = alpha[i]
    hi = oracle.solve_batch(A, rhs, c, cones, eps=1e-10, max_iters=200000)
    assert (hi["status"] == 1).all()
    dx = np.zeros((B, nv)); dx[:, :m] = w
    adj = oracle.adjoint_batch(A, rhs, c, cones, hi["x"], hi["y"], hi["s"], dx, np.zeros_like(hi["y"]), mode="dense")
    g_budget = adj["db"][:, 0]
    g_invp = np.stack([-adj["dA"][:, 1 + i, i] for i in range(m)], axis=1)
    g_alpha = np.stack([(adj["dA"][:, 1 + 2 * m + 3 * i, m + i] + adj["dA"][:, 1 + 2 * m + 3 * i + 2, 2 * m + i]).sum() for i in range(m)])          # (alpha is shared by the batch)
    return hi["x"][:, :m], (g_budget, g_invp, g_alpha)


def test_refine_steps_through_the_layer_on_an_exponential_cone_template():
    """notebook_cases.resource_allocation_template (10 exponential cones, per-instance A) through CvxpyLayer at eps = 1e-4 with two refinement steps: no
    refine_steps warning, the served path, outputs and gradients closer to the oracle's eps = 1e-10 point / dense adjoint than without the steps"""
    from cvxpylayers_amd.interfaces import mi355_if
    from cvxpylayers_amd.torch import CvxpyLayer
    inputs = _resource_inputs()
    m, B, params = inputs
    w = np.random.default_rng(5).standard_normal((B, m))
    y_hi, g_hi = _oracle_reference(inputs, w)

    def run(args):
        layer = CvxpyLayer(template=nc.resource_allocation_template(m), solver_args=args)
        ps = [torch.tensor(p).cuda().requires_grad_() for p in params]
        (yv,) = layer(*ps)
        (yv * torch.from_numpy(w).cuda()).sum().backward()
        torch.cuda.synchronize()
        ey = np.abs(yv.detach().cpu().numpy() - y_hi).max()
        eg = max(np.abs(p.grad.cpu().numpy() - g).max() / (1 + np.abs(g).max()) for p, g in zip(ps, g_hi))
        return ey, eg, layer.info
    mi355_if._WARNED.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        ey1, eg1, info1 = run({"eps": 1e-4, "refine_steps": 2})
        ey0, eg0, info0 = run({"eps": 1e-4})
    assert not [str(x.message) for x in rec if "refine_steps" in str(x.message)]
    assert info1["refine"]["path"] == "ns" and "refine" not in info0
    st = info1["refine"]["status"].cpu().numpy()
    print(f"refine status {np.bincount(st)}; max |y - oracle|: refined {ey1:.3e} unrefined {ey0:.3e}; gradient error: refined {eg1:.3e} unrefined {eg0:.3e}")
    assert ey1 < ey0 and eg1 < eg0


def test_refine_steps_zero_is_bit_identical_to_no_argument():
    """recipe of test_gpu_refine.py::test_off_means_off on exp_pow_mixed: the solver's outputs and the gradients of its value rows"""
    from cvxpylayers_amd.interfaces.mi355_if import MI355_ctx, _CvxpyLayer
    n, cones, A, b, c, _ = K.problem("exp_pow_mixed")
    tpl = P.dense_template(n, cones)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    ctx = MI355_ctx(None, tpl.problem_data_index, cones, options={"eps": 1e-4})
    w = torch.from_numpy(np.random.default_rng(2).standard_normal((A.shape[0], n))).cuda()
    got = []
    for args in ({}, {"refine_steps": 0}, {}):
        A_t, q_t = torch.from_numpy(A_eval).cuda().requires_grad_(), torch.from_numpy(q_eval).cuda().requires_grad_()
        primal, dual, info, _ = _CvxpyLayer.apply(None, q_t, A_t, ctx, args, True, None)
        (primal * w).sum().backward()
        assert "refine" not in info
        got.append((primal.detach(), dual.detach(), A_t.grad, q_t.grad))
    for k, name in enumerate(("primal", "dual", "dA", "dq")):
        print(name, "no argument vs refine_steps=0: max |difference|", float((got[0][k] - got[1][k]).abs().max()), "; two runs without the argument:", float((got[0][k] - got[2][k]).abs().max()))
    for a, g in zip(got[0], got[1]):
        assert torch.equal(a, g)
    # (two solves of one instance agree bit for bit only since k_fwd2 starts the triples' root state from 0: it used to read that LDS uninitialised)
    for a, g in zip(got[0], got[2]):
        assert torch.equal(a, g)


def test_forward_ad_with_jvp_mode_direct_says_direct():
    from cvxpylayers_amd.torch import CvxpyLayer
    m, B, params = _resource_inputs()
    layer = CvxpyLayer(template=nc.resource_allocation_template(m), solver_args={"eps": 1e-9, "max_iters": 200000, "jvp_mode": "direct"})
    ps = [torch.tensor(p).cuda() for p in params]
    gen = torch.Generator(device="cpu").manual_seed(5)
    ts = [0.01 * torch.randn(p.shape, generator=gen, dtype=torch.float64).cuda() for p in ps]
    with fwAD.dual_level():
        (yd,) = layer(*[fwAD.make_dual(p.clone(), t) for p, t in zip(ps, ts)])
        yt = fwAD.unpack_dual(yd).tangent
        info = layer.info["jvp"]
        print("status", info["status"].cpu().numpy(), "iters", info["iters"].cpu().numpy())
        assert info["path"] == "direct" and yt is not None and torch.isfinite(yt).all() and float(yt.abs().max()) > 0
        assert ((info["status"] == 0) == (info["iters"] == 0)).all()          # solved by the elimination, or handed to the re-solve and iterated there
        (yl,) = layer(*[fwAD.make_dual(p.clone(), t) for p, t in zip(ps, ts)], solver_args={"jvp_mode": "lsqr"})
        assert layer.info["jvp"]["path"] == "lsqr"

"""LPGD stated in numpy on top of the oracle (lpgd_kit.py), checked against what is known without a GPU: two one-line sign checks, the adjoint on a box QP
(piecewise-linear solution map: the derived bound), and the order of convergence to the adjoint on a second-order-cone shape.  Seeds and steps were fixed on
the CPU so that the oracle alone meets every condition.

The box QP is problems.native_box_qp_batch -- the nonnegative-cone-only statement of problems.box_qp_batch's data (the same F, g, lo, hi; box_qp_batch itself
carries the objective in a second-order-cone block, whose solution map is not piecewise linear).  The reference is oracle.adjoint_batch in its "dense" mode: its
default LSQR stops at 1e-8, which is far above the bound.  All three modes and all of dA, db, dc, dP are held to the issue's bound alone.  A one-sided difference
of the bilinear G_A, G_P carries the second-order term Dy Dx^T / tau = tau y' x'^T beyond the adjoint, which shrinks with tau while the bound grows as 1 / tau:
tau = 3e-7 puts it (about 1e-5 here) below the bound (about 1e-3 (delta_0 + delta_tau) / 3e-7) with room, and no active set changes at that step."""
import numpy as np
import pytest

import lpgd_kit as lk
from cvxpylayers_amd import problems as P

OPTS = dict(eps=1e-10, max_iters=400000)


@pytest.mark.parametrize("mode", lk.MODES)
def test_sign_checks(mode):
    one = np.ones((1, 1, 1))
    # min 1/2 x^2 - theta x (x <= 100 inactive), loss = x: d loss / d theta = 1, and c = -theta
    g = lk.oracle_lpgd(one, np.array([[100.0]]), np.array([[-0.7]]), {"z": 0, "l": 1, "q": []}, np.ones((1, 1)), np.zeros((1, 1)), 0.1, 0.0, mode, P=one, **OPTS)
    assert abs(-g["dc"][0, 0] - 1.0) < 1e-7, g["dc"]
    # min 1/2 x^2 s.t. x = b, loss = y (= -b): d loss / d b = -1
    g = lk.oracle_lpgd(one, np.array([[0.4]]), np.zeros((1, 1)), {"z": 1, "l": 0, "q": []}, np.zeros((1, 1)), np.ones((1, 1)), 0.1, 0.0, mode, P=one, **OPTS)
    assert abs(g["db"][0, 0] + 1.0) < 1e-7, g["db"]


def _point_error(solve, ref):
    """the oracle's own solution error at a point: the distance to a re-solve at eps / 100"""
    fine = solve(eps=OPTS["eps"] / 100, warm=(ref["x"], ref["y"], ref["s"]))
    return np.maximum(np.abs(ref["x"] - fine["x"]).max(axis=1), np.abs(ref["y"] - fine["y"]).max(axis=1))


@pytest.mark.parametrize("mode", lk.MODES)
def test_box_qp_lpgd_equals_the_adjoint_within_the_derived_bound(mode):
    from oracle import oracle
    nx, B, seed, tau = 6, 16, 1, 3e-7
    A1, b, q, P1, _, _ = P.native_box_qp_batch(nx, B, seed=seed)
    cones = {"z": 0, "l": 2 * nx, "q": []}
    A, Pm = np.broadcast_to(A1, (B,) + A1.shape).copy(), np.broadcast_to(P1, (B, nx, nx)).copy()
    rng = np.random.default_rng(seed + 100)
    dx, dy = rng.standard_normal((B, nx)), rng.standard_normal((B, 2 * nx))
    base = oracle.solve_batch(A, b, q, cones, P=Pm, **OPTS)
    assert (base["status"] == 1).all()
    d0 = _point_error(lambda **kw: oracle.solve_batch(A, b, q, cones, P=Pm, max_iters=400000, **kw), base)
    adj = oracle.adjoint_batch(A, b, q, cones, base["x"], base["y"], base["s"], dx, dy, P=Pm, mode="dense")
    g = lk.oracle_lpgd(A, b, q, cones, dx, dy, tau, 0.0, mode, P=Pm, base=base, **OPTS)
    dt = np.zeros(B)
    cls0 = lk.cone_class(base["y"] - base["s"], cones)
    for sg, ref in g["points"]["pts"].items():
        assert (ref["status"] == 1).all()
        assert (lk.cone_class(ref["y"] - ref["s"], cones) == cls0).all(), "tau is not small enough: an active set changed"
        b_t, c_t, P_t = lk.perturbed_data(b, q, Pm, base["x"], dx, dy, sg * tau, 0.0)
        dt = np.maximum(dt, _point_error(lambda **kw: oracle.solve_batch(A, b_t, c_t, cones, P=P_t, max_iters=400000, **kw), ref))
    bound = lk.point_bound(base["x"], base["y"], d0, dt, tau)
    for key in ("dA", "db", "dc", "dP"):
        err = np.abs(g[key] - adj[key])
        worst = (err.reshape(B, -1).max(axis=1) / bound).max()
        print(f"{mode} {key}: max error / bound = {worst:.3f} (bound {bound.min():.2e} .. {bound.max():.2e})")
        assert worst <= 1.0, (mode, key, worst)
    assert np.abs(adj["dc"]).max() > 1e-2 and np.abs(adj["db"]).max() > 1e-2          # (the comparison is not between zeros)


def test_soc_shape_converges_to_the_adjoint_at_the_order_of_the_difference():
    """n = 12, {z: 2, l: 6, q: [4, 5]}: the error against adjoint_batch at tau and tau / 2 falls by a factor in [1.6, 2.5] for the one-sided modes (order 1) and by
    at least 3 for the central one (order 2).  The error is the Frobenius norm over (dA, db, dc) of the instances kept; an instance whose cone classification of
    y - s differs between the base and a perturbed point is left out, at most 10 % of the batch (seed 2, tau = 4e-3: none is)."""
    from oracle import oracle
    n, cones = lk.SOC_SHAPE
    B, seed, tau = 32, 2, 4e-3
    opts = dict(eps=1e-11, max_iters=400000)
    A, b, c = P.generate(n, cones, B, seed=seed)
    rng = np.random.default_rng(seed + 100)
    dx, dy = rng.standard_normal((B, n)), rng.standard_normal((B, A.shape[1]))
    base = oracle.solve_batch(A, b, c, cones, **opts)
    assert (base["status"] == 1).all()
    adj = oracle.adjoint_batch(A, b, c, cones, base["x"], base["y"], base["s"], dx, dy, mode="dense")
    cls0 = lk.cone_class(base["y"] - base["s"], cones)
    keep, errs = np.ones(B, bool), {}
    for t in (tau, tau / 2):
        for mode in lk.MODES:
            g = lk.oracle_lpgd(A, b, c, cones, dx, dy, t, 0.0, mode, base=base, **opts)
            for ref in g["points"]["pts"].values():
                keep &= (lk.cone_class(ref["y"] - ref["s"], cones) == cls0).all(axis=1) & (ref["status"] == 1)
            errs[mode, t] = np.concatenate([(g[k] - adj[k]).reshape(B, -1) for k in ("dA", "db", "dc")], axis=1)
    assert keep.mean() >= 0.9, keep
    for mode in lk.MODES:
        ratio = np.linalg.norm(errs[mode, tau][keep]) / np.linalg.norm(errs[mode, tau / 2][keep])
        print(f"{mode}: error falls by {ratio:.2f} from tau = {tau} to {tau / 2} ({int(keep.sum())} of {B} instances)")
        assert (ratio >= 3.0) if mode == "lpgd" else (1.6 <= ratio <= 2.5), (mode, ratio)

"""Newton refinement on templates with PSD blocks AND exponential / power triples: k_backward_ns<..., FWD, REF, ..., TRI, ..., PSD> behind ce_refine_psd_tri
(ce_psd_tri_ns_variant >= 0), ConeEngine.refine(psd_ns=True).  The recipes of test_gpu_psd_ns_refine.py on shapes of psd_tri_ns_kit.SHAPES: y-hat of a triple from
its cold-start decision and y-hat of a block from its decomposition inside one acceptance test, the PSD kind's shortened steps.  The starting point is the
engine's own solve at eps = 1e-4 (once per shape, never changed).  Checked against a dense numpy Newton step where the full step is kept (the bounds of
test_gpu_refine._check_step_bounds), the safeguard with rho recomputed in extended precision, the oracle's eps = 1e-10 point after three steps, and a skipped
instance."""
import numpy as np
import pytest
import torch

import psd_tri_ns_kit as K
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from test_gpu_refine import _assert_never_worse, _check_step_bounds, _solve_start, _step_errors

pytestmark = pytest.mark.gpu
_CACHE: dict = {}


def _refine(r, steps, status="given", pt=None):
    """(x, y, s, status, steps, resid_before, resid_after) as numpy arrays of `steps` ce_refine_psd_tri steps from the start (clones: the start stays what it is)"""
    x, y, s = (t.clone() for t in (pt or r["pt"]))
    x, y, s, info = r["eng"].refine(r["A_bm"], r["q_t"], x, y, s, steps, status=r["status"] if isinstance(status, str) else status, psd_ns=True)
    assert info["path"] == "ns"
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (x, y, s, info["status"], info["steps"], info["resid_before"], info["resid_after"]))


def _shape(name):
    """the shape's problem, its eps = 1e-4 start on the GPU, one and three refinement steps from it and the oracle's eps = 1e-10 point: once, shared, not changed"""
    if name not in _CACHE:
        n, cones, A, b, c, hi = K.problem(name)
        r = _solve_start(P.dense_template(n, cones), A, b, c)
        assert _lib.lib().ce_psd_tri_ns_variant(r["eng"]._h) == K.PLAN[name][0]
        r["cones"], r["hi"] = cones, hi
        r["one"], r["three"] = _refine(r, 1), _refine(r, 3)
        _CACHE[name] = r
    return _CACHE[name]


def _solved(r):
    return r["status"].cpu().numpy() >= 0


@pytest.mark.parametrize("shape", ["mix_small", "mix_all", "logdet_like"])
def test_one_step_is_a_dense_newton_step_where_the_full_step_is_kept(shape):
    """fails on a build without the mixed mode: ce_refine_psd_tri does not exist there"""
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
    print("well conditioned", ok.mean(), "reference accepts", acc[ok].mean(), "kernel kept", kept[ok].mean(), "status counts", np.bincount(st),
          "reference rejects", np.flatnonzero(ok & ~acc), "kernel rejected", np.flatnonzero((st & 2) != 0), "kernel flagged", np.flatnonzero((st & 4) != 0))
    both = ok & acc & kept          # (where the reference's full step lowers the residual the kernel's first trial, alpha = 1, is the one it keeps)
    assert both.mean() >= 0.8, both.mean()
    _check_step_bounds(_step_errors(r, dxr, dvr, both), "one step vs numpy")


@pytest.mark.parametrize("shape", ["mix_all", "logdet_like"])
@pytest.mark.parametrize("steps", ["one", "three"])
def test_never_worse(shape, steps):
    r = _shape(shape)
    st = _assert_never_worse(r["np"], r[steps])
    solved = _solved(r)
    assert (((st & 16) == 0) == solved).all() and ((st[solved] & 7) != 0).all()          # failed instances are skipped; every other one took a step, was rejected or was flagged
    rn = K.rho(r["A"], r["b"], r["c"], *r[steps][:3])
    assert (rn <= r[steps][5] * (1 + 1e-9) + 1e-15)[solved].all()          # rho recomputed in extended precision agrees that nothing grew


@pytest.mark.parametrize("shape", ["mix_all", "logdet_like"])
def test_three_steps_land_closer_to_the_oracle_point(shape):
    """distance of the whole point (x, y, s) to the oracle's eps = 1e-10 point, max norm: smaller after three steps than before on EVERY instance"""
    r = _shape(shape)
    hi = r["hi"]
    solved = _solved(r) & (hi["status"] == 1)
    assert solved.all()
    def dist(pt):
        return np.max([np.abs(g - hi[k]).max(axis=1) for g, k in zip(pt, "xys")], axis=0)
    d0, d3 = dist(r["np"]), dist(r["three"][:3])
    st, r0, r1 = r["three"][3], r["three"][5], r["three"][6]
    print(f"{shape}: status counts {np.bincount(st)}; steps kept {np.bincount(r['three'][4])}; resid before median {np.nanmedian(r0):.2e}, after median {np.nanmedian(r1):.2e} "
          f"max {np.nanmax(r1):.2e}; distance before median {np.median(d0):.2e} max {d0.max():.2e}, after median {np.median(d3):.2e} max {d3.max():.2e}; "
          f"not closer: {np.flatnonzero(~(d3 < d0))}")
    assert (d3 < d0).all(), (d0, d3, st)


def test_a_failed_instance_is_skipped_bit_for_bit():
    """mix_all from its eps = 1e-4 start with instance 5 given the forward status -4: status 16 alone, NaN residuals, its point bit for bit; every other instance
    ends exactly where the run without it put it"""
    r = _shape("mix_all")
    x0, y0, s0 = r["np"]
    failed = 5
    status = r["status"].clone(); status[failed] = -4
    out = _refine(r, 3, status=status)
    st = out[3]
    assert st[failed] == 16 and out[4][failed] == 0 and np.isnan(out[5][failed]) and np.isnan(out[6][failed])
    for got, start in zip(out[:3], (x0, y0, s0)):
        assert np.array_equal(got[failed], start[failed])
    others = np.ones(st.size, bool); others[failed] = False
    assert (st[others] == r["three"][3][others]).all()
    for k in range(3):
        assert np.array_equal(out[k][others], r["three"][k][others])


def test_without_the_flag_refine_returns_path_none_as_today():
    r = _shape("mix_small")
    x, y, s = (t.clone() for t in r["pt"])
    x1, y1, s1, info = r["eng"].refine(r["A_bm"], r["q_t"], x, y, s, 2, status=r["status"])
    assert info == {"status": None, "steps": None, "resid_before": None, "resid_after": None, "path": "none"}
    torch.cuda.synchronize()
    for a, b in zip((x1, y1, s1), r["pt"]):
        assert torch.equal(a, b)

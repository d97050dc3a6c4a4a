"""Newton refinement on templates with PSD blocks: k_backward_ns<..., FWD, REF, ..., PSD> behind ce_refine_psd (ce_psd_ns_variant >= 0),
ConeEngine.refine(psd_ns=True).  The recipes of test_gpu_tri_refine.py on shapes of psd_ns_kit.SHAPES, with the dense D and y-hat of a block from
numpy.linalg.eigh: the starting point is the engine's own solve at eps = 1e-4 (once per shape, never changed).  Checked against a dense numpy Newton step (the
bounds of test_gpu_tri_refine.py: test_gpu_refine._check_step_bounds), the safeguard (with the PSD mode's shortened step where the full one fails it), the oracle's eps = 1e-10 point after three steps, a planted stiff block
(stepped, not flagged), a skipped instance, and today's answer without the flag."""
import numpy as np
import pytest
import torch

import psd_ns_kit as K
from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P
from test_gpu_refine import _assert_never_worse, _check_step_bounds, _solve_start, _step_errors

pytestmark = pytest.mark.gpu
_CACHE: dict = {}


def _refine(r, steps, status="given", pt=None):
    """(x, y, s, status, steps, resid_before, resid_after) as numpy arrays of `steps` ce_refine_psd steps from the start (clones: the start stays what it is)"""
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
        assert _lib.lib().ce_psd_ns_variant(r["eng"]._h) == K.host_plan(n, cones)["psd_ns_variant"] >= 0
        r["cones"], r["hi"] = cones, hi
        r["one"], r["three"] = _refine(r, 1), _refine(r, 3)
        _CACHE[name] = r
    return _CACHE[name]


def _pair(v, cones):
    """(y-hat, s-hat) of one v: the complementary pair the residual is evaluated at"""
    yh, _ = K.proj(v, cones)
    return yh, yh - v


def _solved(r):
    return r["status"].cpu().numpy() >= 0


@pytest.mark.parametrize("shape", ["psd_small", "psd_mixed", "lqr_like"])
def test_one_step_is_a_dense_newton_step(shape):
    """fails on a build without the PSD mode: ce_refine_psd does not exist there"""
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
    for i in np.flatnonzero(ok & ~acc):
        print(f"  instance {i}: rho at the start {K.rho(A[i:i + 1], b[i:i + 1], c[i:i + 1], x0[i:i + 1], *(t[None] for t in _pair(v0[i], cones)))[0]:.3e}, after the dense "
              f"full step {K.rho(A[i:i + 1], b[i:i + 1], c[i:i + 1], (x0[i] + dxr[i])[None], *(t[None] for t in _pair(v0[i] + dvr[i], cones)))[0]:.3e}")
    both = ok & acc & kept
    assert both.mean() >= 0.8, both.mean()
    _check_step_bounds(_step_errors(r, dxr, dvr, both), "one step vs numpy")


@pytest.mark.parametrize("shape", ["psd_mixed", "lqr_like"])
@pytest.mark.parametrize("steps", ["one", "three"])
def test_never_worse(shape, steps):
    r = _shape(shape)
    st = _assert_never_worse(r["np"], r[steps])
    solved = _solved(r)
    assert (((st & 16) == 0) == solved).all() and ((st[solved] & 7) != 0).all()          # failed instances are skipped; every other one took a step, was rejected or was flagged
    rn = K.rho(r["A"], r["b"], r["c"], *r[steps][:3])
    assert (rn <= r[steps][5] * (1 + 1e-9) + 1e-15)[solved].all()          # rho recomputed in extended precision agrees that nothing grew


@pytest.mark.parametrize("shape", ["psd_mixed", "lqr_like"])
def test_three_steps_land_closer_to_the_oracle_point(shape):
    """distance of the whole point (x, y, s) to the oracle's eps = 1e-10 point, max norm: smaller after three steps than before on every instance; the median rho
    of the returned points below 1e-14.

    Measured on the MI355X.  psd_mixed: all 48 closer (distance median 4.1e-4 -> 5.1e-10, max 1.1e-2 -> 3.5e-8), median rho 3.9e-16; lqr_like: all 32 closer
    (median 3.7e-4 -> 8.6e-10, max 1.7e-2 -> 1.7e-8), median rho 5.7e-16.  Instance 12 of psd_mixed is the one that needs the PSD mode's shortened step: the full
    Newton step from its eps = 1e-4 point raises rho (8.6e-5 -> 2.2e-4, the dense numpy step alike: test_one_step_is_a_dense_newton_step prints "reference
    rejects [12]"), a shorter one along the same direction lowers it, and the two steps after that are full ones."""
    r = _shape(shape)
    hi = r["hi"]
    solved = _solved(r) & (hi["status"] == 1)
    assert solved.all()
    def dist(pt):
        return np.max([np.abs(g - hi[k]).max(axis=1) for g, k in zip(pt, "xys")], axis=0)
    d0, d3 = dist(r["np"]), dist(r["three"][:3])
    st, r0, r1 = r["three"][3], r["three"][5], r["three"][6]
    print(f"{shape}: status counts {np.bincount(st)}; resid before median {np.nanmedian(r0):.2e}, after median {np.nanmedian(r1):.2e} max {np.nanmax(r1):.2e}; "
          f"distance before median {np.median(d0):.2e} max {d0.max():.2e}, after median {np.median(d3):.2e} max {d3.max():.2e}; not closer: {np.flatnonzero(~(d3 < d0))}")
    assert (d3 < d0).all(), (d0, d3, st)
    assert np.median(r1) < 1e-14, np.median(r1)


def test_a_planted_stiff_block_is_stepped_and_a_failed_instance_is_skipped():
    """psd_mixed from its eps = 1e-4 start: instance 3's first block replaced by U diag(1, 1, -3e-7) U^T (two weighted rows with 1 - B = 3e-7 < NS_TRI_STIFF), instance
    5 given the forward status -4.  The refinement does not apply the stiff rule: instance 3 is not flagged (no bit 4) and is stepped (bit 1: measured, three steps
    kept, rho 0.33 -> 0.049 from a planted point that is no solution).  Instance 5 is skipped: status 16 alone, its
    point bit for bit.  Every other instance ends exactly where the unplanted run put it."""
    r = _shape("psd_mixed")
    x0, y0, s0 = r["np"]
    inst, failed = 3, 5
    y1, s1 = K.plant_stiff_block(y0, s0, r["cones"], inst)
    assert K.block_states(y1[inst] - s1[inst], r["cones"])[1] < 1e-5
    status = r["status"].clone(); status[failed] = -4
    out = _refine(r, 3, status=status, pt=(r["pt"][0], torch.from_numpy(y1).cuda(), torch.from_numpy(s1).cuda()))
    st = out[3]
    print("planted instance: status", st[inst], "steps", out[4][inst], "rho before", out[5][inst], "after", out[6][inst])
    assert st[inst] == 1 and out[4][inst] > 0 and out[6][inst] < out[5][inst], (st[inst], out[4][inst])
    assert st[failed] == 16 and np.isnan(out[5][failed]) and np.isnan(out[6][failed])
    for got, start in zip(out[:3], (x0, y1, s1)):
        assert np.array_equal(got[failed], start[failed])
    others = np.ones(st.size, bool); others[[inst, failed]] = False
    assert (st[others] == r["three"][3][others]).all()
    for k in range(3):
        assert np.array_equal(out[k][others], r["three"][k][others])


def test_without_the_flag_refine_returns_path_none_as_today():
    r = _shape("psd_small")
    x, y, s = (t.clone() for t in r["pt"])
    x1, y1, s1, info = r["eng"].refine(r["A_bm"], r["q_t"], x, y, s, 2, status=r["status"])
    assert info == {"status": None, "steps": None, "resid_before": None, "resid_after": None, "path": "none"}
    torch.cuda.synchronize()
    for a, b in zip((x1, y1, s1), r["pt"]):
        assert torch.equal(a, b)
